#!/usr/bin/env python3
"""CPU emulation of the Float32 dissipation pullback (csrc/ins_temp_adjoint_kernels.h, diss_ubar) and of its Float32 forward
(csrc/ins_temp32.hip, k32t_diffusion + k_dissipation_interp<D, float>): the kernels' formulas in numpy with the metric tables and the inputs cast
to float32 and every operation in float32, against the same formulas in float64.  No GPU: the figures say what Float32 rounding alone does
to the pullback's longer chain (it recomputes diffusion(u) and applies diffusionᵀ to wbar ⊙ u) relative to the forward, on the geometries
of tests/test_gpu_temp_adjoint32.py, whose docstring records them.
    python tools/temp_adjoint32_emulate.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ins_oracle as o  # noqa: E402
from tests import fixtures as fx  # noqa: E402

EPS = np.finfo(np.float64).eps


def box70(o):
    x = (np.linspace(0.0, 7.0, 71), np.linspace(0.0, 6.6, 67), np.linspace(0.0, 0.4, 5))
    d = (o.DirichletBC(), o.DirichletBC())
    return o.make_setup(x, (d, d, (o.PeriodicBC(), o.PeriodicBC())), Re=1000.0)


GEOMS = {
    "setup2d": fx.setup2d, "setup3d": fx.setup3d, "mixed": fx.setup_mixed,
    "periodic3d": lambda o: fx.setup_periodic(o, (12, 10, 8), D=3), "periodic2d": lambda o: fx.setup_periodic(o, (24, 18), D=2), "box70": box70,
}


def shift(a, b, s):
    """a[I + s e_b] with zeros shifted in (only masked-out volumes ever read them)."""
    out = np.zeros_like(a)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if s > 0:
        src[b], dst[b] = slice(s, None), slice(None, -s)
    else:
        src[b], dst[b] = slice(None, s), slice(-s, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def box_mask(N, R):
    m = np.zeros(N, dtype=bool)
    m[tuple(slice(lo, hi) for lo, hi in R)] = True
    return m


def tables(g, b, ga, T):
    """r, ma, mb of direction b for component ga, per index along b (the reads of k32t_diffusion), as arrays broadcast along b"""
    n = g.N[b]
    dx, dxu = np.asarray(g.dx[b], dtype=np.float64), np.asarray(g.dxu[b], dtype=np.float64)
    with np.errstate(divide="ignore"):
        mdx = np.where(dx > 2 * EPS, 1.0 / dx, 0.0)
        mdxu = np.where(dxu > 2 * EPS, 1.0 / dxu, 0.0)
    r = 1.0 / (dxu if ga == b else dx)
    ma, mb = np.zeros(n), np.zeros(n)
    i = np.arange(1, n - 1)
    if ga == b:
        ma[i], mb[i] = mdx[i], mdx[i + 1]
    else:
        ma[i], mb[i] = mdxu[i - 1], mdxu[i]
    shape = [1] * g.D
    shape[b] = n
    return tuple(t.astype(T).reshape(shape) for t in (r, ma, mb))  # rounded to T where they enter the arithmetic


def run(so, T, u64, cbar64):
    """(forward dissipation(u), pullback J(u)^T cbar) in precision T"""
    g = so.grid
    D, N = g.D, tuple(g.N)
    Tq = so.temperature
    visc, coef = T(1.0 / so.Re), T(so.Re * Tq.a1 / Tq.gamma)
    hc = T(0.5) * coef
    u, cbar = u64.astype(T), cbar64.astype(T)
    ip = box_mask(N, g.Ip)
    q = np.where(ip, cbar, T(0))
    fwd = np.zeros(N, dtype=T)
    ubar = np.zeros(N + (D,), dtype=T)
    for ga in range(D):
        dofm = box_mask(N, [(max(lo, 1), min(hi, n - 1)) for (lo, hi), n in zip(g.Iu[ga], N)])
        ua = u[..., ga]
        wb = np.where(dofm, hc * (q + shift(q, ga, 1)), T(0))
        z = wb * ua
        d = np.zeros(N, dtype=T)
        v = np.zeros(N, dtype=T)
        for b in range(D):
            r, ma, mb = tables(g, b, ga, T)
            d = d + visc * ((shift(ua, b, 1) - ua) * mb - (ua - shift(ua, b, -1)) * ma) * r
        d = np.where(dofm, d, T(0))
        v = v + wb * d
        for b in range(D):
            r, ma, mb = tables(g, b, ga, T)
            v = v - visc * z * r * (ma + mb)
            v = v + visc * shift(z * r * mb, b, -1)
            v = v + visc * shift(z * r * ma, b, 1)
        ubar[..., ga] = v
        fwd = fwd + np.where(ip, coef * (shift(ua * d, ga, -1) + ua * d) / T(2), T(0))
    return fwd, ubar


def relmax(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b)))


def main():
    worst = 0.0
    for name, mk in GEOMS.items():
        so = mk(o)
        D = so.grid.D
        bcs = tuple((o.PeriodicBC(), o.PeriodicBC()) if isinstance(a, o.PeriodicBC) else (o.DirichletBC(1.0), o.DirichletBC(0.25))
                    for a, _ in so.boundary_conditions)
        so.temperature = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=bcs, gdir=D - 1)
        so.Re = 1.0 / so.temperature.a1
        N = tuple(so.grid.N)
        u = np.round(fx.randn_field(N + (D,), 11) * 1024.0) / 1024.0
        cbar = np.round(fx.randn_field(N, 13) * 1024.0) / 1024.0
        f64, p64 = run(so, np.float64, u, cbar)
        f32, p32 = run(so, np.float32, u, cbar)
        ef, ep = relmax(f32, f64), relmax(p32, p64)
        worst = max(worst, ep / ef)
        print(f"{name:12s} forward {ef:.3e}  pullback {ep:.3e}  ratio {ep / ef:.2f}")
    print(f"largest pullback / forward ratio {worst:.2f}")


if __name__ == "__main__":
    main()
