#!/usr/bin/env python3
"""Time `create_les_data_ensemble` against the loop of B `create_les_data` calls it replaces (2-D periodic, RK44, fp64, both filters,
nles = (ndns/4, ndns/2), savefreq = 10, no burn-in).

For every ndns in 64, 128, 256 and B in 4, 16, 64, in one process:
  ensemble : one `create_les_data_ensemble(ntrajectory=B, …)` call
  loop     : B `create_les_data(…)` calls sharing one rng — `create_les_data` is unchanged by the ensemble route, so this is the code a user has without it
  stepping : the time steps of either route alone, in the same batches of `savefreq` steps (`timesteps_ensemble_` on B members; B times `timesteps_`), on
             fields and caches made outside the window; what a whole call takes beyond it is the save chain, the set-up and the host copies
Wall time (`time.perf_counter`, the device synchronised before and after): the calls contain blocking device-to-host copies, which is what a user waits
for.  One warm-up run per figure, then `--reps` windows; the median is reported with the min .. max spread, per saved state.  Records go to `--out`
(JSON lines), a table to stdout.
    python tools/les_data_ensemble_time.py --out profiles/les_data_ensemble_time.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins  # noqa: E402

DT = 1e-4


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


def stats(s, per):
    return dict(median=1e3 * statistics.median(s) / per, min=1e3 * min(s) / per, max=1e3 * max(s) / per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--savefreq", type=int, default=10)
    ap.add_argument("--saves", type=int, default=5, help="saved states after the initial one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no other path"
    method = ins.RKMethods.RK44()
    nstep, nsaved = a.saves * a.savefreq, a.saves + 1
    records = []
    for n in a.sizes:
        kw = dict(D=2, Re=2000.0, lims=(0.0, 1.0), nles=(n // 4, n // 2), ndns=n, filters=(ins.FaceAverage(), ins.VolumeAverage()), tburn=0.0,
                  tsim=nstep * DT, savefreq=a.savefreq, Δt=DT)
        setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=2000.0)
        ps = ins.psolver_spectral(setup)
        for B in a.batches:
            fields = [ins.random_field(setup, 0.0, psolver=ps, seed=b) for b in range(B)]
            U = ins.vectorfields(setup, B)
            for b in range(B):
                U[b].copy_(fields[b])
            ens = ins.EnsembleCache(method, setup, ps, B)
            caches = [ins.ode_method_cache(method, setup, ps) for _ in range(B)]
            steppers = [ins.create_stepper(method, setup=setup, psolver=ps, u=u) for u in fields]

            def step_ensemble():
                for _ in range(a.saves):
                    ins.timesteps_ensemble_(ens, U, 0.0, DT, a.savefreq)

            def step_loop():
                for b in range(B):
                    for _ in range(a.saves):
                        ins.timesteps_(method, steppers[b], DT, a.savefreq, cache=caches[b])

            def run_ensemble():
                return ins.create_les_data_ensemble(ntrajectory=B, rng=np.random.default_rng(0), **kw)

            def run_loop():
                rng = np.random.default_rng(0)
                return [ins.create_les_data(rng=rng, **kw) for _ in range(B)]

            te, tl = stats(timed(run_ensemble, a.reps), nsaved), stats(timed(run_loop, a.reps), nsaved)
            se, sl = stats(timed(step_ensemble, a.reps), nsaved), stats(timed(step_loop, a.reps), nsaved)
            rec = dict(ndns=n, nles=list(kw["nles"]), B=B, savefreq=a.savefreq, saved_states=nsaved, steps=nstep, reps=a.reps, ensemble_ms_per_saved_state=te,
                       loop_ms_per_saved_state=tl, ensemble_stepping_ms_per_saved_state=se, loop_stepping_ms_per_saved_state=sl,
                       ensemble_share_beyond_stepping=1.0 - se["median"] / te["median"], loop_share_beyond_stepping=1.0 - sl["median"] / tl["median"],
                       loop_over_ensemble=tl["median"] / te["median"])
            records.append(rec)
            print(f"ndns={n:4d} B={B:3d}: ensemble {te['median']:.3f} ms/saved state ({te['min']:.3f} .. {te['max']:.3f}), stepping alone {se['median']:.3f} "
                  f"({100 * rec['ensemble_share_beyond_stepping']:.0f} % beyond it) | loop {tl['median']:.3f} ({tl['min']:.3f} .. {tl['max']:.3f}), stepping alone "
                  f"{sl['median']:.3f} ({100 * rec['loop_share_beyond_stepping']:.0f} % beyond it) | loop/ensemble = {rec['loop_over_ensemble']:.2f}", flush=True)
            if a.out:  # line by line: a run that is cut short keeps what it measured
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            del ens, U, caches, steppers, fields


if __name__ == "__main__":
    main()
