#!/usr/bin/env python3
"""An ensemble of decaying 2-D turbulence runs: B random solenoidal initial fields of one periodic box advanced together, ONE native call
(`timesteps_ensemble_`) between two observations — every launch of the Runge-Kutta loop works on all B members, which is what a 64² .. 256² grid needs
to keep the card busy — and the ensemble-mean energy spectrum through the ordinary `observespectrum` on each member `U[b]`.
    python examples/DecayingTurbulenceEnsemble2D.py n=128 B=16 tend=0.5"""
import numpy as np

import _common  # noqa: F401
import ins_amd as ins


def main(n=128, B=8, tend=0.2, dt=1e-3, nobs=4, Re=2000.0, kp=6, seed=0, verbose=True):
    setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=Re)
    psolver = ins.psolver_spectral(setup)
    U = ins.vectorfields(setup, B)
    for b in range(B):  # a member is an ordinary vector field of the setup
        U[b].copy_(ins.random_field(setup, 0.0, kp=kp, psolver=psolver, seed=seed + b))
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), setup, psolver, B)

    def observe(t):
        specs = [ins.observespectrum(dict(u=U[b], temp=None, t=t, n=0), setup=setup) for b in range(B)]
        E = [ins.total_kinetic_energy(U[b], setup) for b in range(B)]
        return specs[0]["κ"], np.mean([s["ehat"].value for s in specs], axis=0), E

    nsteps = max(1, round(tend / dt / nobs))
    t = 0.0
    κ, ehat0, E0 = observe(t)
    history = [(t, float(np.mean(E0)))]
    ehat = ehat0
    for _ in range(nobs):
        ins.timesteps_ensemble_(cache, U, t, dt, nsteps)  # all members, nsteps steps, one call
        t += nsteps * dt
        κ, ehat, E = observe(t)
        history.append((t, float(np.mean(E))))
        if verbose:
            print(f"t = {t:.4f}: <E> = {history[-1][1]:.5e}, spectrum peak at κ = {κ[np.argmax(ehat)]}")
    return dict(κ=κ, ehat0=ehat0, ehat=ehat, E0=E0, E=E, energy=history, t=t, maxdiv=max(ins.max_abs_divergence(U[b], setup) for b in range(B)), U=U)


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=128, B=8, tend=0.2, dt=1e-3, nobs=4, Re=2000.0, kp=6, seed=0)))
    print(f"<E>: {r['energy'][0][1]:.5e} -> {r['energy'][-1][1]:.5e} at t = {r['t']:.4f} over {len(r['E'])} members; max|div u| = {r['maxdiv']:.2e}")
