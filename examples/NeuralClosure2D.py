#!/usr/bin/env python3
"""Closure modelling end to end (the pipeline of lib/NeuralClosure in the reference): run a 2-D periodic DNS, filter it onto a coarse grid
with both filters every few steps to get (ū, c) pairs, fit a small CNN to the commutator error c a-priori, and compare the LES with and
without the fitted closure against the filtered DNS a-posteriori.
    python examples/NeuralClosure2D.py ndns=128 nles=32 niter=200
`main(dtype=torch.float32)` runs the whole pipeline in Float32: DNS, filters, stored data, network and the a-posteriori LES."""
import numpy as np
import torch

import _common  # noqa: F401
import ins_amd as ins


def main(ndns=128, nles=32, Re=2000.0, tburn=0.02, tsim=0.1, dt=1e-3, savefreq=2, niter=50, lr=1e-3, seed=0, verbose=True, dtype=torch.float64):
    single = dtype == torch.float32
    rng = np.random.default_rng(seed)
    filters = (ins.FaceAverage(), ins.VolumeAverage())
    procs = dict(log=ins.timelogger(nupdate=20)) if verbose else {}
    data = ins.create_les_data(D=2, Re=Re, lims=(0.0, 1.0), nles=[nles], ndns=ndns, filters=filters, tburn=tburn, tsim=tsim, savefreq=savefreq,
                               Δt=dt, processors=procs, rng=rng, dtype=dtype)
    axis = np.linspace(0.0, 1.0, nles + 1)
    les = ins.Setup(x=(axis, axis), Re=Re)
    psolver = ins.f32.psolver_spectral32(les) if single else ins.psolver_spectral(les)
    io = ins.create_io_arrays(data, les)  # samples of both filters
    x, y = torch.as_tensor(io["u"], device=les.device), torch.as_tensor(io["c"], device=les.device)

    m = ins.cnn(setup=les, radii=[2, 2], channels=[8, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=seed, dtype=dtype)
    with torch.no_grad():
        m.convs[-1].weight.zero_()  # start from "no closure"
    relerr_prior = ins.create_relerr_prior(m, x, y)
    prior_before = relerr_prior(None)
    loader = ins.create_dataloader_prior((io["u"], io["c"]), batchsize=min(16, x.shape[-1]), device=les.device, dtype=dtype)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    ins.train(dataloader=loader, loss=ins.create_loss_prior(m), trainstate=dict(opt=opt, θ=None, rng=rng), niter=niter)
    prior_after = relerr_prior(None)

    # a-posteriori on the face-averaged trajectory: LES steps of savefreq·dt against the filtered DNS states
    method = ins.RKMethods.RK44()
    traj = dict(u=data[0]["u"], t=data[0]["t"])
    post = {}
    for name, closure in (("post_noclosure", None), ("post_cnn", ins.wrappedclosure(m, les))):
        post[name] = ins.create_relerr_post(data=traj, setup=les, method=method, psolver=psolver, closure_model=closure)(None)
    return dict(u=io["u"], c=io["c"], nsample=int(x.shape[-1]), prior_before=prior_before, prior_after=prior_after, **post)


if __name__ == "__main__":
    r = main(**_common.cli(dict(ndns=128, nles=32, Re=2000.0, tburn=0.02, tsim=0.1, dt=1e-3, savefreq=2, niter=50, lr=1e-3, seed=0)))
    print(f"{r['nsample']} samples; a-priori relative error {r['prior_before']:.4f} -> {r['prior_after']:.4f}; "
          f"a-posteriori relative error without closure {r['post_noclosure']:.4e}, with the CNN {r['post_cnn']:.4e}")
