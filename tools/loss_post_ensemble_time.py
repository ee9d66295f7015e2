#!/usr/bin/env python3
"""Time one a-posteriori loss evaluation with its backward, `loss(batch, θ).backward()`, on the ensemble route (`create_loss_post_ensemble`: all B
trajectories in one unrolled graph) against the loop it replaces (`create_loss_post`: `for traj in data`, unchanged by the ensemble route, so this is the
code a user has without it).  2-D periodic LES grids, RK44, fp64, nunroll = 5, the CNN of examples/NeuralClosurePost2D.py: `batched=True` in the ensemble
route (all members one sample in the convolutions; `--unbatched-cnn` switches that off), the plain network in the loop.

For every nles in 32, 64, 128 and B in 4, 16, 64, in one process, on one synthetic batch (random solenoidal start fields, their closure-free trajectories as
reference): wall time (`time.perf_counter`, the device synchronised before and after) of loss + backward; one warm-up per figure, then `--reps` windows;
the median is reported with the min .. max spread.  Records go to `--out` (JSON lines), a table to stdout.
    python tools/loss_post_ensemble_time.py --out profiles/loss_post_ensemble_time.jsonl
`--route ensemble|loop --once` runs a single configuration without timing: one warm-up evaluation, then `--evals` evaluations — what a kernel trace of the
launch count per evaluation wraps."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import ins_amd as ins  # noqa: E402
from NeuralClosurePost2D import closure_cnn  # noqa: E402

DT = 1e-3


def timed(fn, reps):
    """seconds of fn() per call: one warm-up, then `reps` windows of wall time with the device idle at both ends."""
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def stats(s):
    return dict(median=1e3 * statistics.median(s), min=1e3 * min(s), max=1e3 * max(s))


def make_batch(setup, ps, method, B, nunroll):
    U = ins.vectorfields(setup, B)
    for b in range(B):
        U[b].copy_(ins.random_field(setup, 0.0, psolver=ps, seed=b))
    cache = ins.EnsembleCache(method, setup, ps, B)
    states = [U.clone()]
    for _ in range(nunroll):
        ins.timesteps_ensemble_(cache, U, 0.0, DT, 1)
        states.append(1.01 * U)
    t = DT * np.arange(nunroll + 1)
    return [dict(u=torch.stack([s[b] for s in states], dim=-1), t=t) for b in range(B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[32, 64, 128])
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--nunroll", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route", choices=["both", "ensemble", "loop"], default="both")
    ap.add_argument("--once", action="store_true", help="no timing: one warm-up evaluation, then --evals evaluations (for a kernel trace)")
    ap.add_argument("--evals", type=int, default=1)
    ap.add_argument("--unbatched-cnn", action="store_true", help="the ensemble route with the plain CNN (torch's per-sample float64 convolution)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no other path"
    method = ins.RKMethods.RK44()
    records = []
    for n in a.sizes:
        setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=2000.0)
        ps = ins.psolver_spectral(setup)
        m = closure_cnn(setup, batched=not a.unbatched_cnn)  # the ensemble route's network: all members one sample in the convolutions
        m_loop = closure_cnn(setup, batched=False)  # the loop's: the network as a user has it without the ensemble route (same seed, same weights)
        params = list(m.parameters()) + list(m_loop.parameters())
        losses = dict(ensemble=ins.create_loss_post_ensemble(setup=setup, method=method, psolver=ps, closure_model=ins.wrappedclosure_ensemble(m, setup)),
                      loop=ins.create_loss_post(setup=setup, method=method, psolver=ps, closure_model=ins.wrappedclosure(m_loop, setup)))
        for B in a.batches:
            batch = make_batch(setup, ps, method, B, a.nunroll)

            def evaluate(route):
                for q in params:
                    q.grad = None
                losses[route](batch, None).backward()

            routes = ["ensemble", "loop"] if a.route == "both" else [a.route]
            if a.once:
                for r in routes:
                    evaluate(r)
                    torch.cuda.synchronize()
                    for _ in range(a.evals):
                        evaluate(r)
                    torch.cuda.synchronize()
                    print(f"nles {n} B {B} route {r}: 1 warm-up + {a.evals} evaluation(s) done")
                continue
            rec = dict(nles=n, B=B, nunroll=a.nunroll, method="RK44", reps=a.reps, unit="ms per loss(...).backward()", ensemble_cnn_batched=not a.unbatched_cnn)
            for r in routes:
                rec[r] = stats(timed(lambda: evaluate(r), a.reps))
            if len(routes) == 2:
                rec["loop_over_ensemble"] = rec["loop"]["median"] / rec["ensemble"]["median"]
            records.append(rec)
            print("  ".join(f"{k}={v if not isinstance(v, dict) else {q: round(x, 3) for q, x in v.items()}}" for k, v in rec.items()), flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
