#!/usr/bin/env python3
"""CPU emulation of the Float32 Smagorinsky closure (csrc/ins_smagforce32.hip): the numpy oracle's smagtensor! -> apply_bc_p! -> divoftensor!
(operators.jl:1135-1150, 1203-1236, 1284-1300) with the metric tables and the input cast to float32 and every operation in float32, against
the same chain in float64 on the same float32-representable input.  No GPU: the figures say what Float32 rounding alone does to the closure
force — a square root of a sum of squares of differences, then a difference of products — on the grids of tests/test_gpu_closure32.py, whose
bounds they confirm (an emulated error under a quarter of the 2e-5 operator bound of the Float32 tests lets that bound stand).
    python tools/closure32_emulate.py"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ins_oracle as o  # noqa: E402
from tests import fixtures as fx  # noqa: E402

THETA = 0.17
OP_BOUND = 2e-5


def exact_box(o, n, Re=500.0):  # tests/test_gpu_f32.py
    return o.make_setup(tuple(np.arange(ni + 1) * 2.0**-6 for ni in n), Re=Re)


def lid(o, n=(24, 16, 12)):  # tests/test_gpu_f32.py, _lid_setup
    x = (o.cosine_grid(0.0, 1.0, n[0]), o.cosine_grid(0.0, 1.0, n[1]), np.linspace(-0.2, 0.2, n[2] + 1))
    D = o.DirichletBC
    return o.make_setup(x, ((D(), D()), (D(), D((1.0, 0.0, 0.2))), (o.PeriodicBC(), o.PeriodicBC())), Re=1000.0)


def symuniform3d(o):  # tests/test_gpu_fields.py
    x = (np.linspace(0.0, 1.0, 67), np.linspace(0.0, 0.5, 9), np.linspace(0.0, 0.25, 8))
    S, P = o.SymmetricBC, o.PeriodicBC
    return o.make_setup(x, ((S(), S()), (P(), P()), (S(), S())), Re=1000.0)


def symmetric3d(o):  # tests/test_gpu_fields.py
    x = (o.tanh_grid(0.0, 1.0, 14, 1.2), o.cosine_grid(0.0, 1.0, 9), o.tanh_grid(0.0, 0.5, 10, 1.1))
    S, Dr = o.SymmetricBC, o.DirichletBC
    return o.make_setup(x, ((S(), S()), (S(), Dr()), (Dr(), S())), Re=1000.0)


def periodic_box(n):
    return lambda o: o.make_setup(tuple(np.linspace(0.0, L, ni + 1) for ni, L in zip(n, (1.0, 0.7, 1.3))), Re=1000.0)


def walled(case):
    """The wall-bounded and stretched boxes of the one-kernel against three-kernel test."""

    def mk(o):
        Dr, Sy, Pe, Pr = o.DirichletBC, o.SymmetricBC, o.PeriodicBC, o.PressureBC
        if case == "walls":
            x = (o.tanh_grid(0.0, 1.0, 72, 1.2), o.cosine_grid(0.0, 1.0, 12), o.tanh_grid(0.0, 0.5, 10, 1.1))
            bc = ((Dr(), Dr((0.3, 0.0, 0.1))), (Dr(), Dr((1.0, 0.2, 0.0))), (Dr(), Dr()))
        elif case == "channel":
            x = (np.linspace(0.0, 2.0, 138), o.tanh_grid(0.0, 1.0, 10, 1.5), o.cosine_grid(0.0, 0.8, 9))
            bc = ((Pe(), Pe()), (Dr(), Dr()), (Sy(), Sy()))
        elif case == "mixed":
            x = (o.cosine_grid(0.0, 1.0, 61), np.linspace(0.0, 0.7, 17), o.tanh_grid(0.0, 1.3, 70, 1.3))
            bc = ((Sy(), Dr()), (Pe(), Pe()), (Dr(), Sy()))
        elif case == "outflow":
            x = (o.tanh_grid(0.0, 2.0, 72, 1.2), o.cosine_grid(0.0, 1.0, 12), np.linspace(0.0, 0.5, 11))
            bc = ((Dr((1.0, 0.0, 0.0)), Pr()), (Sy(), Sy()), (Dr(), Pr()))
        elif case == "symuniform":
            x = (np.linspace(0.0, 1.0, 71), np.linspace(0.0, 0.5, 13), np.linspace(0.0, 0.25, 11))
            bc = ((Sy(), Sy()), (Pe(), Pe()), (Sy(), Sy()))
        else:  # tiny
            x = (np.linspace(0.0, 1.0, 6), np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 7))
            bc = ((Dr(), Dr()), (Dr(), Sy()), (Sy(), Dr()))
        return o.make_setup(x, bc, Re=1000.0)

    return mk


GEOMS = {
    "periodic2d": lambda o: fx.setup_periodic(o, (24, 18), D=2), "periodic3d": lambda o: fx.setup_periodic(o, (12, 10, 8), D=3),
    "wide3d": lambda o: exact_box(o, (128, 16, 16)), "dirichlet2d": fx.setup2d, "dirichlet3d": fx.setup3d, "mixed3d": fx.setup_mixed, "lid3d": lid,
    "symmetric3d": symmetric3d, "symuniform3d": symuniform3d,
    "per(64,9,4)": periodic_box((64, 9, 4)), "per(61,16,70)": periodic_box((61, 16, 70)), "per(5,4,6)": periodic_box((5, 4, 6)),
    "per(136,20,37)": periodic_box((136, 20, 37)),
    **{c: walled(c) for c in ("walls", "channel", "mixed", "tiny", "symuniform", "outflow")},
}


def cast_setup(so, T):
    """A copy of the oracle setup whose metric tables are rounded to T (the kernels round a table entry where it enters the arithmetic)."""
    s = copy.copy(so)
    s.grid = copy.copy(so.grid)
    for name in ("dx", "dxu"):
        setattr(s.grid, name, tuple(np.asarray(a).astype(T) for a in getattr(so.grid, name)))
    return s


def closure(so, T, u64):
    """(σ on Ip, closure force) with every operation in precision T"""
    s = cast_setup(so, T)
    g = s.grid
    D, R = g.D, g.Ip
    u = u64.astype(T)
    G = o.gradu(u, s).astype(T)  # formed in T from T operands; the oracle stores it in a float64 array, exactly
    S = (G + np.swapaxes(G, -1, -2)) / T(2)
    d2 = T(0)
    for a in range(D):
        d2 = d2 + o._vec(g.dx[a], R[a], a, D) ** 2
    eddy = T(THETA) * T(THETA) * d2 * np.sqrt(T(2) * np.sum(S * S, axis=(-1, -2), dtype=T))
    sig = np.zeros(tuple(g.N) + (D, D), dtype=T, order="F")
    sig[o._sl(R)] = T(2) * eddy[..., None, None] * S
    assert sig.dtype == T and eddy.dtype == T
    for i in range(D):
        for j in range(D):
            comp = np.asfortranarray(sig[..., i, j])
            o.apply_bc_p_(comp, 0.0, s)
            sig[..., i, j] = comp
    out = np.zeros(tuple(g.N) + (D,), dtype=T, order="F")
    o.divoftensor_(out, sig, s)
    return sig, out


def relmax(a, b):
    return float(np.max(np.abs(a.astype(np.float64) - b)) / np.max(np.abs(b)))


def rell2(a, b):
    return float(np.sqrt(np.sum((a.astype(np.float64) - b) ** 2)) / np.sqrt(np.sum(b**2)))


def main():
    worst = 0.0
    for name, mk in GEOMS.items():
        so = mk(o)
        g = so.grid
        u = o.apply_bc_u(np.asfortranarray(fx.randn_field(tuple(g.N) + (g.D,), 1).astype(np.float32).astype(np.float64)), 0.0, so)
        u = np.asfortranarray(u.astype(np.float32).astype(np.float64))
        s64, f64 = closure(so, np.float64, u)
        s32, f32 = closure(so, np.float32, u)
        assert f32.dtype == np.float32
        es, ef = relmax(s32, s64), relmax(f32, f64)
        worst = max(worst, es, ef)
        print(f"{name:16s} smagtensor relmax {es:.3e}   closure force relmax {ef:.3e} rell2 {rell2(f32, f64):.3e}")
    print(f"largest emulated error {worst:.3e}; a quarter of the operator bound {OP_BOUND / 4:.1e}: the bound {'stands' if worst < OP_BOUND / 4 else 'is exceeded'}")


if __name__ == "__main__":
    main()
