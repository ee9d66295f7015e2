"""Times of the DNS-to-LES filters on periodic 3-D boxes: face and volume average, tiled and generic kernel, next to the same
result written as torch ops on the padded tensor (strided slices + `avg_pool3d` / `mean`: the baseline, not the code under test) and to a flat
device copy of the same box; then one `filtersaver` update against one DNS step.  One JSON line per measurement; median (and min / max) of
`--reps` event-timed repetitions after `--warmup`.  "compulsory" bytes: 3·8·n³/comp (face), 3·8·n³·(comp+1)/comp (volume); half of that for
the Float32 kernels (csrc/ins_filter32.hip), which `--dtype float32` times on the rounded field in the same run, every line tagged with its dtype
(the torch-ops baseline is timed in float64 only).

    python tools/filter_time.py [--n 256 512] [--comp 2 4 8] [--dtype float64 float32] [--reps 20] [--warmup 3]
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
    return statistics.median(ts), min(ts), max(ts)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def torch_face(u, c):
    """The face average as torch ops on the padded tensor (x fastest: the tensor is viewed z, y, x)."""
    out = []
    for a in range(3):
        w = u[..., a].permute(2, 1, 0)[1:-1, 1:-1, 1:-1]  # (z, y, x) interior
        k = [c, c, c]
        k[2 - a] = 1
        sl = [slice(None)] * 3
        sl[2 - a] = slice(c - 1, None, c)
        out.append(torch.nn.functional.avg_pool3d(w[tuple(sl)][None, None], tuple(k))[0, 0])
    return out


def torch_volume(u, c):
    """The volume average (even comp) as torch ops: periodic pad by comp/2 along α, then a (comp+1)-wide window with stride comp."""
    h = c // 2
    out = []
    for a in range(3):
        w = u[..., a].permute(2, 1, 0)[1:-1, 1:-1, 1:-1]
        d = 2 - a
        w = torch.cat([w.narrow(d, c - h - 1, w.shape[d] - (c - h - 1)), w.narrow(d, 0, c - h)], dim=d)  # fine planes c−h … n+c−h of the periodic extension
        k = [c, c, c]
        k[d] = c + 1
        out.append(torch.nn.functional.avg_pool3d(w[None, None], tuple(k), stride=c)[0, 0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--comp", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--saver-n", type=int, default=256)
    ap.add_argument("--dtype", nargs="+", default=["float64", "float32"], choices=["float64", "float32"])
    a = ap.parse_args()
    f32 = ins.f32
    torch.cuda.set_device(0)
    for n in a.n:
        dns = ins.Setup(x=tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3)), Re=1000.0, device="cuda:0")
        u64 = ins.random_field(dns, 0.0, seed=1)
        fields = {"float64": u64, "float32": f32.to_f32(dns, u64)}
        for dt in a.dtype:
            u = fields[dt]
            u2 = ins.copyfield(u)
            ms, lo, hi = timed(lambda: u2.copy_(u), a.reps, a.warmup)
            emit(what="flat_copy", dtype=dt, n=n, ms=ms, min_ms=lo, max_ms=hi, GBps=2 * u.numel() * u.element_size() / ms / 1e6)
            del u2
        for c in a.comp:
            les = ins.Setup(x=tuple(np.linspace(0.0, 1.0, n // c + 1) for _ in range(3)), Re=1000.0, device="cuda:0")
            for kind, Φ, nbytes in (("face", ins.FaceAverage(), 24.0 * n**3 / c), ("volume", ins.VolumeAverage(), 24.0 * n**3 * (c + 1) / c)):
                for dt in a.dtype:  # both precisions of one case back to back
                    u = fields[dt]
                    v = f32.vectorfield32(les) if dt == "float32" else ins.vectorfield(les)
                    for name, off in (("tiled", 0), ("generic", 1)):
                        with ins._lib.options(INS_DISABLE_FILTER_TILED=off):
                            ms, lo, hi = timed(lambda: Φ(v, u, les, c, setup_dns=dns), a.reps, a.warmup)
                        emit(what=f"{kind}_{name}", dtype=dt, n=n, comp=c, ms=ms, min_ms=lo, max_ms=hi,
                             compulsory_GBps=nbytes * u.element_size() / 8 / ms / 1e6)
                if "float64" not in a.dtype:
                    continue
                u, v = u64, ins.vectorfield(les)
                tf = torch_face if kind == "face" else torch_volume
                ref = tf(u, c)
                got = Φ(v, u, les, c, setup_dns=dns)
                err = max(float((ref[q] - got[..., q].permute(2, 1, 0)[1:-1, 1:-1, 1:-1]).abs().max()) for q in range(3))
                ms, lo, hi = timed(lambda: tf(u, c), a.reps, a.warmup)
                emit(what=f"{kind}_torch_ops", dtype="float64", n=n, comp=c, ms=ms, min_ms=lo, max_ms=hi, compulsory_GBps=nbytes / ms / 1e6, max_diff_vs_kernel=err)
                del ref, got
            del les, v
        del u, u64, fields, dns
        torch.cuda.empty_cache()
    # one filtersaver update (momentum + bc + project on the DNS grid, filter u and F, LES right-hand side, two downloads) against one DNS step
    n, c = a.saver_n, 4
    dns = ins.Setup(x=tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3)), Re=1000.0, device="cuda:0")
    les = ins.Setup(x=tuple(np.linspace(0.0, 1.0, n // c + 1) for _ in range(3)), Re=1000.0, device="cuda:0")
    method = ins.RKMethods.RK44()
    u64 = ins.random_field(dns, 0.0, psolver=ins.psolver_spectral(dns), seed=2)
    for dt in a.dtype:
        if dt == "float32":
            ps, psl, u = f32.psolver_spectral32(dns), f32.psolver_spectral32(les), f32.to_f32(dns, u64)
            cache = f32.ERKCache32(method, dns, ps)
            ms, lo, hi = timed(lambda: f32.timestep32_(cache, u, 1e-4), a.reps, a.warmup)
        else:
            ps, psl, u = ins.psolver_spectral(dns), ins.psolver_spectral(les), ins.copyfield(u64)
            cache = ins.ode_method_cache(method, dns, ps)
            st = ins.create_stepper(method, setup=dns, psolver=ps, u=u)
            ms, lo, hi = timed(lambda: ins.timestep_(method, st, 1e-4, cache=cache), a.reps, a.warmup)
        emit(what="dns_rk44_step", dtype=dt, n=n, ms=ms, min_ms=lo, max_ms=hi)
        for kind, Φ in (("face", ins.FaceAverage()), ("volume", ins.VolumeAverage())):
            saver = ins.filtersaver(dns, [les], [Φ], [c], ps, [psl], nupdate=1)
            state = dict(u=u, temp=None, t=0.0, n=0)
            saver.initialize(lambda: state)
            ms, lo, hi = timed(lambda: saver.on_step(state), a.reps, a.warmup)
            emit(what=f"filtersaver_update_{kind}", dtype=dt, n=n, comp=c, ms=ms, min_ms=lo, max_ms=hi)


if __name__ == "__main__":
    main()
