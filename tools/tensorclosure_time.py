"""Times of the tensor-basis closure on 3-D periodic boxes, in one process on one box:

  (i)  `ins.tensorbasis` + a torch contraction Σ_i a_i B_i — the only route there was before the fused kernels (11·9 + 5 fields stored);
  (ii) `tensorinvariants_` + `tensorclosure_stress_` (csrc/ins_tensorclosure.hip: the basis stays in registers);
  and the fused pullback `tensorclosure_pullback_` (stress and invariant cotangents, abar and ubar).

One JSON line per measurement; median of `--reps` event-timed repetitions after `--warmup`.  Algorithmic bytes per cell: 64 (invariants:
u + V), 160 (stress: u + a + τ), 528 (pullback: the three launches' inputs and outputs, the ∇ubar scratch written and read once).

    python tools/tensorclosure_time.py [--n 128 256] [--reps 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ins_amd as ins  # noqa: E402
from ins_amd.setup import _alloc  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def randn(sp, ncomp, seed):
    f = _alloc(sp, tuple(sp.grid.N) + (ncomp,))
    g = torch.Generator(device=sp.device).manual_seed(seed)
    f.copy_(torch.randn(f.shape, generator=g, dtype=torch.float64, device=sp.device))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-unfused", action="store_true", help="route (ii) and the pullback only (profiler runs)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        sp = ins.Setup(x=x, Re=1000.0, device="cuda:0")
        cells = float(np.prod(sp.grid.N))
        u = ins.random_field(sp, 0.0, seed=1)
        coef = randn(sp, 11, 2)
        V, tau = _alloc(sp, tuple(sp.grid.N) + (5,)), ins.tensorfield(sp)

        def gbps(nbytes, ms):
            return nbytes * cells / ms / 1e6

        # (ii) fused
        ms_v = timed(lambda: ins.tensorinvariants_(V, u, sp), a.reps, a.warmup)
        emit(what="tensorinvariants", n=n, ms=ms_v, algorithmic_GBps=gbps(64, ms_v))
        ms_s = timed(lambda: ins.tensorclosure_stress_(tau, u, coef, sp), a.reps, a.warmup)
        emit(what="tensorclosure_stress", n=n, ms=ms_s, algorithmic_GBps=gbps(160, ms_s))
        emit(what="fused_forward_total", n=n, ms=ms_v + ms_s, algorithmic_GBps=gbps(224, ms_v + ms_s))
        # pullback
        taubar, Vbar = randn(sp, 6, 3), randn(sp, 5, 4)
        abar, ubar = _alloc(sp, tuple(sp.grid.N) + (11,)), ins.vectorfield(sp)
        ms_p = timed(lambda: ins.tensorclosure_pullback_(ubar, abar, taubar, Vbar, u, coef, sp), a.reps, a.warmup)
        emit(what="tensorclosure_pullback", n=n, ms=ms_p, algorithmic_GBps=gbps(528, ms_p))
        del taubar, Vbar, abar, ubar
        torch.cuda.empty_cache()
        if not a.skip_unfused:
            # (i) B and V stored, then contracted by torch
            B = _alloc(sp, tuple(sp.grid.N) + (99,))
            ms_b = timed(lambda: ins.tensorbasis_(B, V, u, sp), a.reps, a.warmup)
            emit(what="tensorbasis", n=n, ms=ms_b, algorithmic_GBps=gbps(24 + 8 * 104, ms_b))
            Bm = ins.tensorbasis_matrices(B, sp)
            reps = max(3, a.reps // 4)
            ms_c = timed(lambda: (coef[..., None, None] * Bm).sum(dim=-3), reps, 1)
            emit(what="torch_contraction_mul_sum", n=n, ms=ms_c)
            ms_e = timed(lambda: torch.einsum("...i,...ipq->...pq", coef, Bm), reps, 1)
            emit(what="torch_contraction_einsum", n=n, ms=ms_e)
            ms_i = ms_b + min(ms_c, ms_e)
            emit(what="unfused_forward_total", n=n, ms=ms_i, speedup_of_fused=ms_i / (ms_v + ms_s))
            del B, Bm
        del u, coef, V, tau, sp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
