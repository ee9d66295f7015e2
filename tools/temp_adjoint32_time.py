"""Times of the fused temperature pullback in both precisions on a periodic box (DESIGN.md "Differentiability", "Temperature equation"):
ins_temperature_pullback_f32 (temperature_pullback32_) next to ins_temperature_pullback_f64 (temperature_pullback_) on the same random fields,
with the dissipation term on and off, and a flat read + write copy of as many bytes in each precision.  One JSON line per measurement; median
of `--reps` event-timed repetitions after `--warmup`, all in one process.  Bytes per cell are counted from the stencils of the 3-D fused
entry: u 3 + temp 1 + cbar 1 + Fbar[gdir] 1 read, ubar 3 read + 3 written, tempbar 1 written = 13 values.

    python tools/temp_adjoint32_time.py [--n 256] [--reps 20] [--warmup 3] [--out profiles/temp_adjoint32_time.jsonl]
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

VALUES_PER_CELL = 13


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "w") if a.out else None

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    F = ins.f32
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    for n in a.n:
        x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
        for diss in (True, False):
            T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per, per), dodissipation=diss, gdir=2)
            sp = ins.Setup(x=x, Re=1000.0, temperature=T, device="cuda:0")
            cells = float(np.prod(sp.grid.N))
            u = ins.random_field(sp, 0.0, seed=1)
            Fbar = ins.copyfield(u)
            temp = ins.scalarfield(sp)
            temp.copy_(torch.randn(temp.shape, dtype=torch.float64, device=sp.device, generator=torch.Generator(device=sp.device).manual_seed(2)))
            cbar = ins.copyfield(temp)
            ubar, tempbar = ins.vectorfield(sp), ins.scalarfield(sp)
            u32, Fbar32, temp32, cbar32 = (F.to_f32(sp, f) for f in (u, Fbar, temp, cbar))
            ubar32, tempbar32 = F.vectorfield32(sp), F.scalarfield32(sp)
            tag = dict(n=n, dodissipation=diss)
            for what, size, fn in (
                ("temperature_pullback_f64", 8, lambda: ins.temperature_pullback_(ubar, tempbar, Fbar, cbar, u, temp, sp)),
                ("temperature_pullback_f32", 4, lambda: F.temperature_pullback32_(ubar32, tempbar32, Fbar32, cbar32, u32, temp32, sp)),
            ):
                ms = timed(fn, a.reps, a.warmup)
                emit(what=what, ms=ms, algorithmic_TBps=VALUES_PER_CELL * size * cells / ms / 1e9, **tag)
        # a flat copy that reads and writes as many bytes as the fused entry moves (7 values read, 6 written + ... : 13 values, half each way)
        for what, dtype, size in (("copy_f64", torch.float64, 8), ("copy_f32", torch.float32, 4)):
            nel = int(VALUES_PER_CELL * cells) // 2
            src = torch.empty(nel, dtype=dtype, device="cuda:0").normal_()
            dst = torch.empty_like(src)
            ms = timed(lambda: dst.copy_(src), a.reps, a.warmup)
            emit(what=what, ms=ms, algorithmic_TBps=2 * nel * size / ms / 1e9, n=n)
            del src, dst
    if out:
        out.close()


if __name__ == "__main__":
    main()
