#!/usr/bin/env python3
"""Fitting the Smagorinsky constant through a rollout (the a-posteriori baseline of NeuralClosure's `create_loss_post`): a 16^3 periodic box, RK44,
a target produced with one θ, and a few Adam steps on another θ against it.  Every loss evaluation is one `ins.ad.timesteps(…, θ=θ)` call: the
closure runs inside the native forward loop and inside the native reverse step, ∂L/∂θ comes from the fused closure pullback, and the memory is
that of the checkpoints however long the rollout.
    python examples/SmagorinskyFit3D.py n=16 nsteps=10 iters=6"""
import numpy as np
import torch

import _common  # noqa: F401
import ins_amd as ins


def main(n=16, nsteps=10, dt=1e-2, Re=1e4, theta_target=0.2, theta0=0.1, iters=6, lr=0.02, checkpoint_every=None, verbose=True):
    x = tuple(np.linspace(0.0, 2 * np.pi, n + 1) for _ in range(3))
    setup = ins.Setup(x=x, Re=Re)
    setup.closure_model = ins.smagorinsky_closure(setup)
    psolver = ins.psolver_spectral(setup)
    method = ins.RKMethods.RK44()

    def start(a, x, y, z):  # two superposed Taylor-Green modes: strain everywhere, so the closure acts
        if a == 0:
            return np.sin(x) * np.cos(y) * np.cos(z) + 0.5 * np.sin(2 * x) * np.cos(2 * y) * np.cos(z)
        if a == 1:
            return -np.cos(x) * np.sin(y) * np.cos(z) - 0.5 * np.cos(2 * x) * np.sin(2 * y) * np.cos(z)
        return 0 * (x + y + z)

    u0 = ins.velocityfield(setup, start, psolver=psolver)

    def rollout(θ):
        return ins.ad.timesteps(method, ins.create_stepper(method, setup=setup, psolver=psolver, u=u0), dt, nsteps, θ=θ, checkpoint_every=checkpoint_every).u

    with torch.no_grad():
        target = rollout(theta_target)
        scale = float(((target - rollout(0.0)) ** 2).sum())  # the closure's whole effect on the final field: the loss is 1 at θ = 0
    θ = torch.tensor(theta0, dtype=torch.float64, device=setup.device, requires_grad=True)
    opt = torch.optim.Adam([θ], lr=lr)
    losses, thetas = [], []
    for it in range(iters):
        opt.zero_grad()
        loss = ((rollout(θ) - target) ** 2).sum() / scale
        loss.backward()
        losses.append(float(loss.detach()))
        thetas.append(float(θ.detach()))
        if verbose:
            print(f"iteration {it}: θ = {thetas[-1]:.4f}, loss = {losses[-1]:.6e}, dL/dθ = {float(θ.grad):.6e}")
        opt.step()
    with torch.no_grad():
        losses.append(float(((rollout(float(θ)) - target) ** 2).sum() / scale))
    thetas.append(float(θ.detach()))
    if verbose:
        print(f"after {iters} steps: θ = {thetas[-1]:.4f} (target {theta_target}), loss = {losses[-1]:.6e}")
    return dict(losses=losses, thetas=thetas, theta_target=theta_target)


if __name__ == "__main__":
    main(**_common.cli(dict(n=16, nsteps=10, dt=1e-2, Re=1e4, theta_target=0.2, theta0=0.1, iters=6, lr=0.02)))
