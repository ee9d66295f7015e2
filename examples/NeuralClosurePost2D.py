#!/usr/bin/env python3
"""A-posteriori closure training on an ensemble of trajectories: `create_les_data_ensemble` produces the filtered-DNS data of B seeds in the launches of
one, and `create_loss_post_ensemble` unrolls the LES of all trajectories of a batch as ONE autograd graph (`ad.timestep_ensemble`).  A small CNN that
starts from "no closure" is trained with Adam through the unrolled steps; it is built with `batched=True`, so that its float64 convolutions see all
members as one sample (torch would otherwise convolve sample by sample) and the launch count of a loss evaluation does not depend on the batch size.
    python examples/NeuralClosurePost2D.py ndns=64 nles=32 B=4 nunroll=3 niter=10"""
import numpy as np
import torch

import _common  # noqa: F401
import ins_amd as ins


def closure_cnn(setup, seed=0, batched=True):
    """the example's network: two 5 x 5 convolutions, 8 hidden channels, the last layer zeroed (no closure at the start); `batched`: all samples of a call
    go through the convolutions as one"""
    m = ins.cnn(setup=setup, radii=[2, 2], channels=[8, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=seed, batched=batched)
    with torch.no_grad():
        m.convs[-1].weight.zero_()
    return m


def main(ndns=64, nles=32, B=4, Re=2000.0, tburn=0.02, tsim=0.02, dt=1e-3, savefreq=2, nunroll=3, niter=10, lr=1e-3, seed=0):
    rng = np.random.default_rng(seed)
    data = ins.create_les_data_ensemble(ntrajectory=B, D=2, Re=Re, lims=(0.0, 1.0), nles=(nles,), ndns=ndns, filters=(ins.FaceAverage(),), tburn=tburn,
                                        tsim=tsim, savefreq=savefreq, Δt=dt, rng=rng)
    trajectories = [dict(u=member[0]["u"], t=member[0]["t"]) for member in data]
    axis = np.linspace(0.0, 1.0, nles + 1)
    les = ins.Setup(x=(axis, axis), Re=Re)
    psolver = ins.psolver_spectral(les)
    m = closure_cnn(les, seed)
    loss = ins.create_loss_post_ensemble(setup=les, method=ins.RKMethods.RK44(), psolver=psolver, closure_model=ins.wrappedclosure_ensemble(m, les),
                                         nsubstep=savefreq)
    loader = ins.create_dataloader_post(trajectories, ntrajectory=B, nunroll=nunroll, device=les.device)
    check, _ = loader(np.random.default_rng(seed + 1))  # one fixed batch to compare before and after
    with torch.no_grad():
        before = float(loss(check, None))
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    history = []

    def callback(state, trainstate):
        with torch.no_grad():
            state.append(float(loss(check, None)))
        return state

    ins.train(dataloader=loader, loss=loss, trainstate=dict(opt=opt, θ=None, rng=rng), niter=niter, callback=callback, callbackstate=history)
    return dict(loss_before=before, loss_after=history[-1], history=history, ntrajectory=B, nstate=len(trajectories[0]["t"]))


if __name__ == "__main__":
    r = main(**_common.cli(dict(ndns=64, nles=32, B=4, Re=2000.0, tburn=0.02, tsim=0.02, dt=1e-3, savefreq=2, nunroll=3, niter=10, lr=1e-3, seed=0)))
    print(f"{r['ntrajectory']} trajectories of {r['nstate']} states; a-posteriori loss on a fixed batch {r['loss_before']:.6e} -> {r['loss_after']:.6e}")
