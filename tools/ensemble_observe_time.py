#!/usr/bin/env python3
"""Time of ONE observation of an ensemble (energy, max divergence and CFL step of every member, and every member's energy spectrum), B = 16 and 64 members at
64², 128² and 256²:
  route A  the per-member loop: total_kinetic_energy, max_abs_divergence, get_cfl_timestep_ and observespectrum on each U[b] (3·B blocking reads and B
           spectrum downloads);
  route B  ensemble_stats + observespectrum_ensemble (six launches, the three statistics read once, one spectrum download).
Wall time per observation between device synchronisations, median of `reps` after a warm-up; the launch counts are those of the code paths (see
DESIGN.md §8 item 7a), not measured here.  One JSON line per case, appended to profiles/ensemble_observe_time.jsonl.
    python tools/ensemble_observe_time.py [sizes=64,128,256] [B=16,64] [reps=20] [out=profiles/ensemble_observe_time.jsonl]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(sizes=(64, 128, 256), Bs=(16, 64), reps=20, out=os.path.join(ROOT, "profiles", "ensemble_observe_time.jsonl")):
    import torch

    import ins_amd as ins

    rows = []
    for n in sizes:
        setup = ins.Setup(x=(np.linspace(0.0, 1.0, n + 1),) * 2, Re=2000.0)
        psolver = ins.psolver_spectral(setup)
        for B in Bs:
            U = ins.vectorfields(setup, B)
            for b in range(B):
                U[b].copy_(ins.apply_bc_u_(ins.random_field(setup, 0.0, kp=6, psolver=psolver, seed=b), 0.0, setup))
            cache = ins.EnsembleCache(ins.RKMethods.RK44(), setup, psolver, B)
            obs = [ins.Observable(dict(u=U[b], temp=None, t=0.0, n=0)) for b in range(B)]
            members = [ins.observespectrum(obs[b], setup=setup) for b in range(B)]  # route A's spectrum handles, made once as route B's is

            def route_a():
                for b in range(B):
                    obs[b].value = dict(u=U[b], temp=None, t=0.0, n=0)  # recomputes that member's spectrum and downloads it
                E = [ins.total_kinetic_energy(U[b], setup) for b in range(B)]
                d = max(ins.max_abs_divergence(U[b], setup) for b in range(B))
                c = min(ins.get_cfl_timestep_(None, U[b], setup) for b in range(B))
                return np.mean([m["ehat"].value for m in members], axis=0), E, d, c

            def route_b():
                st = ins.ensemble_stats(cache, U)
                e = ins.observespectrum_ensemble(cache, U)["ehat"]
                s = torch.stack([st["E"], st["maxdiv"], st["Δt_cfl"]]).cpu().numpy()  # one read of the three statistics
                return e.mean(axis=0), s[0], s[1].max(), s[2].min()

            def clock(f):
                for _ in range(3):
                    f()
                ts = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    ts.append(time.perf_counter() - t0)
                return float(np.median(ts)) * 1e3

            a, b_ = route_a(), route_b()
            agree = float(np.max(np.abs(a[0] - b_[0])) / np.max(np.abs(a[0])))
            row = dict(n=n, B=B, reps=reps, per_member_ms=clock(route_a), ensemble_ms=clock(route_b), spectrum_relmax=agree,
                       cfl_equal=bool(a[3] == b_[3]), maxdiv_equal=bool(a[2] == b_[2]), device=torch.cuda.get_device_name(0))
            row["ratio"] = row["per_member_ms"] / row["ensemble_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
            del cache, members, obs
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return rows


if __name__ == "__main__":
    kw = dict(a.split("=", 1) for a in sys.argv[1:])
    main(sizes=tuple(int(s) for s in kw.get("sizes", "64,128,256").split(",")), Bs=tuple(int(s) for s in kw.get("B", "16,64").split(",")),
         reps=int(kw.get("reps", 20)), **({"out": kw["out"]} if "out" in kw else {}))
