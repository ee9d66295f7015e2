#!/usr/bin/env python3
"""Time the ensemble stepper against what it replaces (RK44, 2-D periodic boxes of 64², 128², 256²).

For every size and B in 1, 2, 4, 8, 16, 32, 64, measured in one process on the same fields:
  ensemble : one `timesteps_ensemble_` call of `--steps` steps on B members          -> ms per ensemble step, ms per member-step
  loop     : B `timesteps_` calls of `--steps` steps, one ERKCache and one field each -> the same two figures (the code path a user has without the feature)
and per size the single-field `timesteps_` time (`--single-only` prints nothing else: run it with INS_HIP_LIB pointing at another build of libinship.so,
alternating with this one, to compare the single-field path of two builds).

Device events around each timed window, the stream synchronised before and after; every shape is warmed up first; `--reps` windows per figure, the median
is reported with the min .. max spread.  Records go to `--out` (JSON lines), a table to stdout.
    python tools/ensemble_time.py --steps 200 --reps 5 --out profiles/ensemble_2d_time.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins  # noqa: E402

DT = 1e-4


def timed(fn, reps):
    """ms of fn() per call: `reps` windows between device events."""
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def stats(ms, per):
    return dict(median=statistics.median(ms) / per, min=min(ms) / per, max=max(ms) / per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no other path"
    method = ins.RKMethods.RK44()
    records = []
    for n in a.sizes:
        setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=2000.0)
        ps = ins.psolver_spectral(setup)
        bmax = 1 if a.single_only else max(a.batches)
        fields = [ins.random_field(setup, 0.0, kp=6, psolver=ps, seed=b) for b in range(bmax)]
        caches = [ins.ode_method_cache(method, setup, ps) for _ in range(bmax)]
        steppers = [ins.create_stepper(method, setup=setup, psolver=ps, u=ins.copyfield(u)) for u in fields]

        def loop(B):
            for b in range(B):
                ins.timesteps_(method, steppers[b], DT, a.steps, cache=caches[b])

        loop(1)  # warm-up of the shape
        single = stats(timed(lambda: loop(1), a.reps), a.steps)
        rec = dict(kind="single", n=n, steps=a.steps, reps=a.reps, label=a.label, lib=os.environ.get("INS_HIP_LIB", ""), ms_per_step=single)
        records.append(rec)
        print(f"{n:4d}^2 single-field timesteps_{' [' + a.label + ']' if a.label else ''}: {single['median']:.4f} ms/step "
              f"({single['min']:.4f} .. {single['max']:.4f})", flush=True)
        if a.single_only:
            continue
        for B in a.batches:
            U = ins.vectorfields(setup, B)
            for b in range(B):
                U[b].copy_(fields[b])
            ens = ins.EnsembleCache(method, setup, ps, B)
            ins.timesteps_ensemble_(ens, U, 0.0, DT, a.steps)  # warm-up
            loop(B)
            te = stats(timed(lambda: ins.timesteps_ensemble_(ens, U, 0.0, DT, a.steps), a.reps), a.steps)
            tl = stats(timed(lambda: loop(B), a.reps), a.steps)
            ratio = tl["median"] / te["median"]
            records.append(dict(kind="ensemble", n=n, B=B, steps=a.steps, reps=a.reps, ensemble_ms_per_step=te, loop_ms_per_step=tl,
                                ensemble_ms_per_member_step=te["median"] / B, loop_ms_per_member_step=tl["median"] / B, loop_over_ensemble=ratio,
                                single_ms_per_step=single["median"], ensemble_over_single=te["median"] / single["median"]))
            print(f"{n:4d}^2 B={B:3d}: ensemble {te['median']:.4f} ms/step ({te['min']:.4f} .. {te['max']:.4f}) = {te['median'] / B:.5f} per member-step | "
                  f"loop of {B} timesteps_ {tl['median']:.4f} ms/step ({tl['min']:.4f} .. {tl['max']:.4f}) = {tl['median'] / B:.5f} per member-step | "
                  f"loop/ensemble = {ratio:.2f}, ensemble/single = {te['median'] / single['median']:.2f}", flush=True)
            del ens, U
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
