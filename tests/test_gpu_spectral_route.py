"""Every launch sequence of the spectral Poisson solver (csrc/ins_poisson.hip, SpectralRoute) on its smallest box against the oracle, and the
route as a property of the solver: chosen when it is created, not moved by a switch set afterwards."""
import ctypes

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_parity import POISSON_TOL, ins, mirror, rell2  # noqa: F401  (ins: the module-scoped fixture)
from tests.test_spectral_route import KY_OF, OWN2D, OWN2D_ONE, OWN_LDS, OWN_LINE3, OWN_XY, OWN_YZ, ROCFFT, ROCFFT_ZFUSED

pytestmark = pytest.mark.gpu

YZ = dict(INS_YZ_FUSED=1, INS_YZ_PARTITIONS=2)


def route_of(ps):
    from ins_amd import _lib

    ky, engine = ctypes.c_int32(-2), ctypes.c_int32(-2)
    route = _lib.load().ins_dbg_spectral_route(ps.handle, ctypes.byref(ky))
    _lib.call("ins_poisson_fft_engine", ps.handle, ctypes.byref(engine))
    return route, ky.value, engine.value


def rhs(so, seed=23):
    f = fx.randn_field(so.grid.N, seed)
    ip = tuple(slice(lo, hi) for lo, hi in so.grid.Ip)
    f[ip] -= f[ip].mean()
    return f, ip


@pytest.mark.parametrize("route,n,opts", [(OWN_XY, (16, 16, 16), {}), (OWN_LDS, (128, 32, 16), {}), (OWN_LINE3, (16, 128, 16), {}),
                                          (OWN_YZ, (32, 128, 64), YZ), (ROCFFT_ZFUSED, (24, 20, 16), {}), (ROCFFT, (12, 20, 8), {}),
                                          (OWN2D_ONE, (16, 16), {}), (OWN2D, (128, 16), {})])
def test_each_route_matches_oracle(ins, oracle, route, n, opts):
    from ins_amd import _lib

    o = oracle
    D = len(n)
    so = fx.setup_periodic(o, n, D=D)
    sp = mirror(ins, so, o)
    pso = o.psolver_spectral(so)
    with _lib.options(**opts):
        psp = ins.psolver_spectral(sp)
    assert route_of(psp) == (route, KY_OF[route], 2 if route == ROCFFT_ZFUSED else (0 if route == ROCFFT else 1))
    f, ip = rhs(so)
    want = o.poisson(pso, f)
    got = ins.to_numpy(ins.poisson(psp, ins.from_numpy(sp, f)))
    print(f"route {route} {n}: psolver(p) rel L2 = {rell2(got[ip], want[ip]):.3e}")
    assert rell2(got[ip], want[ip]) < POISSON_TOL
    u_h = o.apply_bc_u(fx.randn_field(so.grid.N + (D,), 24), 0.0, so)
    want_u = o.project_(u_h.copy(order="F"), so, pso, o.scalarfield(so))
    u = ins.from_numpy(sp, u_h)
    ins.project_(u, sp, psp, ins.scalarfield(sp))
    print(f"route {route} {n}: project_ rel L2 = {rell2(ins.to_numpy(u), want_u):.3e}")
    assert rell2(ins.to_numpy(u), want_u) < POISSON_TOL


@pytest.mark.parametrize("n,created_under,route,switch,other", [((32, 32, 32), {}, OWN_XY, dict(INS_DISABLE_XYFUSED=1), OWN_LDS),
                                                                ((32, 128, 64), YZ, OWN_YZ, dict(INS_DISABLE_YZ_FUSED=1), OWN_LINE3)])
def test_route_is_frozen_at_creation(ins, oracle, n, created_under, route, switch, other):
    """A switch set through ins_set_option after the solver exists does not move it: same route, bitwise the same solution.  A solver created under
    the switch takes the other route and agrees to the Poisson tolerance."""
    from ins_amd import _lib

    o = oracle
    so = fx.setup_periodic(o, n, D=3)
    sp = mirror(ins, so, o)
    with _lib.options(**created_under):
        ps = ins.psolver_spectral(sp)
    assert route_of(ps)[0] == route
    f, ip = rhs(so)
    first = ins.to_numpy(ins.poisson(ps, ins.from_numpy(sp, f)))
    with _lib.options(**switch):
        again = ins.to_numpy(ins.poisson(ps, ins.from_numpy(sp, f)))
        assert route_of(ps)[0] == route
        ps2 = ins.psolver_spectral(sp)
        assert route_of(ps2)[0] == other
        second = ins.to_numpy(ins.poisson(ps2, ins.from_numpy(sp, f)))
    assert np.array_equal(first, again)
    print(f"{n}: route {route} against route {other}: rel L2 = {rell2(second[ip], first[ip]):.3e}")
    assert rell2(second[ip], first[ip]) < POISSON_TOL
