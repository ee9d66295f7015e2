#!/usr/bin/env python3
"""CPU emulation of the Float32 observers (csrc/ins_fields_kernels.h with T = float): vorticity!, interpolate_u_p!, interpolate_ω_p! and Qfield!
(operators.jl:985-1020, 1311-1370, 1440-1460) spelled as the kernels spell them — reciprocal metric tables formed in double and rounded to float
where they enter, every operation in float32 — against the same formulas in float64 on the same float32-representable input.  No GPU: the figures
say what Float32 rounding alone does to each observer on the grids of tests/test_gpu_solve32.py, which takes 4 x the emulated maximum as its bound
(the margin of the Float32 pullback tests: it covers reassociation and fused multiply-adds).
    python tools/fields32_emulate.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _take(f, region, shift=None):
    """f over the index box `region` (a (lo, hi) per direction), shifted by `shift` volumes per direction"""
    shift = shift or (0,) * len(region)
    return f[tuple(slice(lo + s, hi + s) for (lo, hi), s in zip(region, shift))]


def _e(D, b, s=1):
    return tuple(s if a == b else 0 for a in range(D))


def _metric(v, region, b, T):
    """1 / v over region[b] as the kernels see it: the reciprocal in double, rounded to T, shaped to broadcast along direction b"""
    lo, hi = region[b]
    shape = [1] * len(region)
    shape[b] = hi - lo
    return (1.0 / np.asarray(v, dtype=np.float64)[lo:hi]).astype(T).reshape(shape)


def vorticity(u, N, dxu, T):
    """(ω on [0, N-1), that box): 2-D a scalar field, 3-D a vector field; zeros elsewhere"""
    D = len(N)
    box = [(0, n - 1) for n in N]
    u = u.astype(T)
    if D == 2:
        w = np.zeros(N, dtype=T)
        w[tuple(slice(lo, hi) for lo, hi in box)] = (_take(u[..., 1], box, _e(2, 0)) - _take(u[..., 1], box)) * _metric(dxu[0], box, 0, T) - (
            _take(u[..., 0], box, _e(2, 1)) - _take(u[..., 0], box)) * _metric(dxu[1], box, 1, T)
        return w, box
    w = np.zeros(tuple(N) + (3,), dtype=T)
    for a in range(3):
        ap, am = (a + 1) % 3, (a + 2) % 3
        w[tuple(slice(lo, hi) for lo, hi in box) + (a,)] = (_take(u[..., am], box, _e(3, ap)) - _take(u[..., am], box)) * _metric(dxu[ap], box, ap, T) - (
            _take(u[..., ap], box, _e(3, am)) - _take(u[..., ap], box)) * _metric(dxu[am], box, am, T)
    return w, box


def interpolate_u_p(u, N, Ip, T):
    D = len(N)
    u = u.astype(T)
    up = np.zeros_like(u)
    for a in range(D):
        up[tuple(slice(lo, hi) for lo, hi in Ip) + (a,)] = (_take(u[..., a], Ip, _e(D, a, -1)) + _take(u[..., a], Ip)) / T(2)
    return up


def interpolate_w_p(w, N, Ip, T):
    D = len(N)
    w = w.astype(T)
    wp = np.zeros_like(w)
    sl = tuple(slice(lo, hi) for lo, hi in Ip)
    if D == 2:
        wp[sl] = (_take(w, Ip, (-1, -1)) + _take(w, Ip)) / T(2)
        return wp
    for a in range(3):
        ap, am = (a + 1) % 3, (a + 2) % 3
        sh = tuple(-1 if b in (ap, am) else 0 for b in range(3))
        wp[sl + (a,)] = (_take(w[..., a], Ip, sh) + _take(w[..., a], Ip)) / T(2)
    return wp


def qfield(u, N, Ip, dx, T):
    D = len(N)
    u = u.astype(T)
    q = np.zeros(tuple(hi - lo for lo, hi in Ip), dtype=T)
    for a in range(D):
        for b in range(D):
            q = q - (_take(u[..., a], Ip) - _take(u[..., a], Ip, _e(D, b, -1))) * _metric(dx[b], Ip, b, T) * (
                _take(u[..., b], Ip) - _take(u[..., b], Ip, _e(D, a, -1))) * _metric(dx[a], Ip, a, T) / T(2)
    Q = np.zeros(N, dtype=T)
    Q[tuple(slice(lo, hi) for lo, hi in Ip)] = q
    return Q


def relmax(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b)))


def emulate(u, N, Ip, dx, dxu):
    """Emulated Float32 rounding error (largest difference over the written range / largest reference magnitude) of the four observers on the
    float32-representable ghost-filled field `u` (float64 array, N + (D,)): dict(vorticity, interpolate_u_p, interpolate_ω_p, Qfield)."""
    N, Ip = tuple(int(n) for n in N), [(int(lo), int(hi)) for lo, hi in Ip]
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))
    out = {}
    w64, box = vorticity(u, N, dxu, np.float64)
    w32, _ = vorticity(u, N, dxu, np.float32)
    assert w32.dtype == np.float32
    sb = tuple(slice(lo, hi) for lo, hi in box)
    out["vorticity"] = relmax(w32[sb], w64[sb])
    sp = tuple(slice(lo, hi) for lo, hi in Ip)
    out["interpolate_u_p"] = relmax(interpolate_u_p(u, N, Ip, np.float32)[sp], interpolate_u_p(u, N, Ip, np.float64)[sp])
    wr = w64.astype(np.float32).astype(np.float64)  # the interpolation's own input, float32-representable
    out["interpolate_ω_p"] = relmax(interpolate_w_p(wr, N, Ip, np.float32)[sp], interpolate_w_p(wr, N, Ip, np.float64)[sp])
    out["Qfield"] = relmax(qfield(u, N, Ip, dx, np.float32)[sp], qfield(u, N, Ip, dx, np.float64)[sp])
    return out


def grids(o):
    """The observer grids of tests/test_gpu_solve32.py as oracle setups: a 2-D stretched box between walls in y, and the mixed sides of
    tests/fixtures.py (Periodic x Dirichlet/Pressure x Symmetric) at up to 34 volumes per side."""
    D, Pe, Pr, Sy = o.DirichletBC, o.PeriodicBC, o.PressureBC, o.SymmetricBC
    return {
        "walls2d 20x12": o.make_setup((o.tanh_grid(0.0, 2.0, 20, 1.2), o.cosine_grid(0.0, 1.0, 12)), ((Pe(), Pe()), (D(), D())), Re=1000.0),
        "mixed3d 34x20x6": o.make_setup((o.tanh_grid(0.0, 5.0, 34), o.cosine_grid(0.0, 1.0, 20), o.tanh_grid(0.0, 0.8, 6)),
                                         ((Pe(), Pe()), (D(), Pr()), (Sy(), Sy())), Re=1000.0),
    }


def test_field(o, so, seed=1):
    """The input of the observer tests: a float32-representable random field with its ghost volumes filled"""
    from tests import fixtures as fx

    g = so.grid
    u = o.apply_bc_u(np.asfortranarray(fx.randn_field(tuple(g.N) + (g.D,), seed).astype(np.float32).astype(np.float64)), 0.0, so)
    return np.asfortranarray(u.astype(np.float32).astype(np.float64))


def main():
    from oracle import ins_oracle as o

    for name, so in grids(o).items():
        g = so.grid
        r = emulate(test_field(o, so), g.N, g.Ip, g.dx, g.dxu)
        print(f"{name:18s} " + "   ".join(f"{k} {v:.3e}" for k, v in r.items()))


if __name__ == "__main__":
    main()
