#!/usr/bin/env python3
"""The ensemble of examples/DecayingTurbulenceEnsemble2D.py run with an adaptive time step: `solve_unsteady_ensemble(Δt=None)` advances all B members with
one Δt, `cfl` times the smallest CFL step of any member (two launches and one host read per adaptation).  Every observation — the members' energies and
max |div u| (`ensemble_stats`) and their spectra (`observespectrum_ensemble`) — costs six launches whatever B is, where the per-member loop of the
fixed-step example costs several hundred at B = 64.
    python examples/DecayingTurbulenceEnsembleAdaptive2D.py n=128 B=16 tend=0.5"""
import numpy as np

import _common  # noqa: F401
import ins_amd as ins


def main(n=128, B=8, tend=0.2, cfl=0.9, n_adapt=4, nupdate=20, Re=2000.0, kp=6, seed=0, verbose=True):
    setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=Re)
    psolver = ins.psolver_spectral(setup)
    U = ins.vectorfields(setup, B)
    for b in range(B):  # a member is an ordinary vector field of the setup
        U[b].copy_(ins.apply_bc_u_(ins.random_field(setup, 0.0, kp=kp, psolver=psolver, seed=seed + b), 0.0, setup))
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), setup, psolver, B)
    history, spectra = [], []

    def observe(V, t, k):
        st = ins.ensemble_stats(cache, V)  # device values of all members; the reads below synchronise
        spec = ins.observespectrum_ensemble(cache, V)
        history.append((t, float(st["E"].mean()), float(st["maxdiv"].max())))
        spectra.append((spec["κ"], spec["ehat"].mean(axis=0)))
        if verbose:
            print(f"n = {k:5d}  t = {t:.4f}: <E> = {history[-1][1]:.5e}, max|div u| = {history[-1][2]:.2e}, spectrum peak at κ = {spec['κ'][np.argmax(spectra[-1][1])]}")

    (U, t), Δts = ins.solve_unsteady_ensemble(cache=cache, U=U, tlims=(0.0, tend), Δt=None, cfl=cfl, n_adapt_Δt=n_adapt, docopy=False, observe=observe,
                                              nupdate=nupdate)
    if len(Δts) % nupdate:  # the end state, when the last step is no multiple of nupdate
        observe(U, t, len(Δts))
    E = ins.ensemble_stats(cache, U)["E"].cpu().numpy().copy()
    return dict(κ=spectra[-1][0], ehat0=spectra[0][1], ehat=spectra[-1][1], E=E, energy=[(t_, e) for t_, e, _ in history], t=t, Δts=Δts,
                maxdiv=max(d for _, _, d in history), U=U)


if __name__ == "__main__":
    r = main(**_common.cli(dict(n=128, B=8, tend=0.2, cfl=0.9, n_adapt=4, nupdate=20, Re=2000.0, kp=6, seed=0)))
    print(f"<E>: {r['energy'][0][1]:.5e} -> {r['energy'][-1][1]:.5e} at t = {r['t']:.4f} in {len(r['Δts'])} steps (Δt {min(r['Δts']):.2e} .. "
          f"{max(r['Δts']):.2e}) over {len(r['E'])} members; max|div u| = {r['maxdiv']:.2e}")
