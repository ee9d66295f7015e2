"""The temperature equation of the `_f32` family (csrc/ins_temp32.hip, ins_rk_step_ext_f32; examples/RayleighBenard3D.jl:16 runs T = Float32) against the
oracle.  The checker is the one of tests/test_gpu_f32.py: the numpy oracle in float64 on the float32-rounded inputs, float32 tolerances.  Emulating Float32
rounding on the CPU (the oracle with metrics and inputs cast to numpy float32 against fp64) gives 0.5-1.9e-7 for these operators on these grids, so the
2e-5 operator bound of the existing Float32 tests leaves two orders of margin."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import fixtures as fx

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def rell2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b**2)), 1e-300))


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _geom(o, name):
    from tests.test_gpu_f32 import _lid_setup, exact_box

    return {"dirichlet2d": fx.setup2d, "dirichlet3d": fx.setup3d, "mixed3d": fx.setup_mixed, "lid3d": _lid_setup,
            "periodic3d": lambda o: fx.setup_periodic(o, (12, 10, 8), D=3), "periodic2d": lambda o: fx.setup_periodic(o, (24, 18), D=2),
            "wide3d": lambda o: exact_box(o, (128, 16, 16))}[name](o)  # wide3d: a box the 64-wide float stage kernel takes


def _setups(ins, o, geom, kind, gdir, diss):
    """Oracle and product setups of `geom` with a temperature equation; Re = 1/α1 (setup.jl:12)."""
    from tests.test_gpu_fields import mirror_temp, temp_bcs
    from tests.test_gpu_parity import mirror

    so = _geom(o, geom)
    T = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=temp_bcs(o, so, kind), gdir=gdir, dodissipation=diss)
    so.temperature = T
    sp = mirror(ins, so, o)
    sp.temperature = mirror_temp(ins, o, T)
    so.Re = sp.Re = 1.0 / T.a1
    return so, sp


def _r32(a):
    return np.asfortranarray(np.asarray(a).astype(np.float32).astype(np.float64))


# every gdir < D and dodissipation both ways; kinds "dirichlet" and "symmetric" on the wall-bounded grids (periodic sides stay periodic)
CASES = [("dirichlet2d", "dirichlet", 1, True), ("dirichlet2d", "symmetric", 0, False), ("dirichlet3d", "dirichlet", 2, True),
         ("dirichlet3d", "symmetric", 1, False), ("mixed3d", "symmetric", 2, True), ("mixed3d", "dirichlet", 0, False), ("lid3d", "dirichlet", 1, True),
         ("lid3d", "symmetric", 0, True), ("periodic3d", "any", 2, True), ("periodic2d", "any", 1, True), ("periodic2d", "any", 0, False),
         ("wide3d", "any", 0, True), ("wide3d", "any", 2, False)]


@pytest.mark.parametrize("geom,kind,gdir,diss", CASES)
def test_temperature_operators_f32_match_oracle(ins, oracle, geom, kind, gdir, diss):
    o, f32 = oracle, ins.f32
    so, sp = _setups(ins, o, geom, kind, gdir, diss)
    g, D = so.grid, so.grid.D
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    # ghost fill: copies and constants, exact in float32
    raw_t = fx.randn_field(g.N, 4).astype(np.float32)
    got = f32.apply_bc_temp32_(f32.to_f32(sp, raw_t), sp).cpu().numpy()
    t_h = o.apply_bc_temp(np.asfortranarray(raw_t.astype(np.float64)), 0.0, so)
    assert np.array_equal(got, t_h.astype(np.float32))
    u_h = o.apply_bc_u(_r32(fx.randn_field(g.N + (D,), 1)), 0.0, so)
    u, t = f32.to_f32(sp, u_h), f32.to_f32(sp, t_h)
    u64, t64 = ins.from_numpy(sp, u_h), ins.from_numpy(sp, t_h)
    c0 = fx.randn_field(g.N, 5).astype(np.float32)
    c0_h = np.asfortranarray(c0.astype(np.float64))
    F0 = fx.randn_field(g.N + (D,), 6).astype(np.float32)
    F0_h = np.asfortranarray(F0.astype(np.float64))
    outside_ip = np.ones(g.N, dtype=bool)
    outside_ip[ip] = False
    figures = {}

    # convection_diffusion_temp! (c += ... on Ip)
    got = f32.convection_diffusion_temp32_(f32.to_f32(sp, c0), u, t, sp).cpu().numpy()
    want = o.convection_diffusion_temp_(c0_h.copy(order="F"), u_h, t_h, so)
    figures["convdiff"] = relmax(got.astype(np.float64), want)
    assert np.array_equal(got[outside_ip], c0[outside_ip])
    k64 = ins.to_numpy(ins.convection_diffusion_temp_(ins.from_numpy(sp, c0_h), u64, t64, sp))
    figures["convdiff vs fp64 kernel"] = relmax(got.astype(np.float64), k64)

    # dissipation! (diss += ... on Ip; diff: diffusion(u) on the degrees of freedom, zero elsewhere, whatever it held)
    diff = f32.to_f32(sp, fx.randn_field(g.N + (D,), 7).astype(np.float32))
    got = f32.dissipation32_(f32.to_f32(sp, c0), diff, u, sp).cpu().numpy()
    diff_h = o.vectorfield(so)
    want = o.dissipation_(c0_h.copy(order="F"), diff_h, u_h, so)
    got_diff = diff.cpu().numpy()
    figures["dissipation"] = relmax(got.astype(np.float64), want)
    figures["diffusion"] = relmax(got_diff.astype(np.float64), diff_h)
    assert np.array_equal(got[outside_ip], c0[outside_ip])
    assert not np.any(got_diff[diff_h == 0.0])  # off the degrees of freedom: the zeros of fill!(diff, 0)
    d64 = ins.vectorfield(sp)
    k64 = ins.to_numpy(ins.dissipation_(ins.from_numpy(sp, c0_h), d64, u64, sp))
    figures["dissipation vs fp64 kernel"] = relmax(got.astype(np.float64), k64)
    figures["diffusion vs fp64 kernel"] = relmax(got_diff.astype(np.float64), ins.to_numpy(d64))

    # gravity! (F[:, gdir] += ... on Iu[gdir])
    got = f32.gravity32_(f32.to_f32(sp, F0), t, sp).cpu().numpy()
    want = o.gravity_(F0_h.copy(order="F"), t_h, so)
    figures["gravity"] = relmax(got.astype(np.float64), want)
    outside_iu = np.ones(g.N + (D,), dtype=bool)
    outside_iu[tuple(slice(lo, hi) for lo, hi in g.Iu[gdir]) + (gdir,)] = False
    assert np.array_equal(got[outside_iu], F0[outside_iu])
    k64 = ins.to_numpy(ins.gravity_(ins.from_numpy(sp, F0_h), t64, sp))
    figures["gravity vs fp64 kernel"] = relmax(got.astype(np.float64), k64)

    # momentum! with the gravity term
    F = f32.vectorfield32(sp)
    F.fill_(7.0)
    got = f32.momentum32_(F, u, sp, temp=t).cpu().numpy().astype(np.float64)
    want = o.momentum_ext_(o.vectorfield(so), u_h, t_h, 0.0, so)
    if geom.startswith(("periodic", "wide")):  # all-periodic boxes: ins_momentum_f32 writes the interior only (tests/test_gpu_f32.py compares Ip)
        got, want = got[ip], want[ip]
    figures["momentum"] = relmax(got, want)

    print(geom, kind, gdir, diss, {k: f"{v:.2e}" for k, v in figures.items()})
    for name, v in figures.items():
        assert v < 2e-5, (name, v)


STEP_CASES = [("dirichlet2d", "dirichlet", 1, True), ("dirichlet3d", "symmetric", 2, True), ("mixed3d", "symmetric", 0, False),
              ("mixed3d", "dirichlet", 2, True), ("lid3d", "dirichlet", 1, True), ("periodic3d", "any", 2, True), ("periodic2d", "any", 0, True),
              ("periodic2d", "any", 1, False), ("wide3d", "any", 1, True)]


@pytest.mark.parametrize("geom,kind,gdir,diss", STEP_CASES)
@pytest.mark.parametrize("method", ["RK44", "Wray3"])
def test_temperature_steps_f32_match_oracle(ins, oracle, geom, kind, gdir, diss, method):
    """Three steps of (u, temp) on the Float32 stage loop (timesteps32_ ×2 then timestep32_) against oracle.timestep_ext_ ×3 from the same
    float32-representable start; the same run operator by operator (INS_DISABLE_TEMP32_STAGE) agrees with the one-pass stage kernel to rounding."""
    from ins_amd import _lib

    o, f32 = oracle, ins.f32
    so, sp = _setups(ins, o, geom, kind, gdir, diss)
    g, D = so.grid, so.grid.D
    pso = o.default_psolver(so)
    u0 = 0.5 * fx.randn_field(g.N + (D,), 31).astype(np.float32).astype(np.float64)
    u0 = o.apply_bc_u(o.project_(o.apply_bc_u(np.asfortranarray(u0), 0.0, so), so, pso, o.scalarfield(so)), 0.0, so)
    u0 = _r32(u0)
    t0 = _r32(o.apply_bc_temp(0.5 + 0.1 * fx.randn_field(g.N, 4), 0.0, so))
    dt = 0.3 * o.get_cfl_timestep(u0, so)
    mo = getattr(o, method)()
    st = dict(setup=so, psolver=pso, u=u0.copy(order="F"), temp=t0.copy(order="F"), t=0.0, n=0)
    oc = o.ode_method_cache_ext(mo, so)
    for _ in range(3):
        st = o.timestep_ext_(mo, st, dt, oc)
    ps = f32.default_psolver32(sp)
    assert isinstance(ps, f32.psolver_wrap32) == (not geom.startswith(("periodic", "wide")))
    cache = f32.ERKCache32(getattr(ins.RKMethods, method)(), sp, ps)

    def run():
        u, t = f32.to_f32(sp, u0), f32.to_f32(sp, t0)
        f32.timesteps32_(cache, u, dt, 2, temp=t)
        ru, rt = f32.timestep32_(cache, u, dt, temp=t)
        assert ru is u and rt is t
        return u, u.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)

    u, gu, gt = run()
    hmin = min(float(np.min(g.dx[a][1:-1])) for a in range(D))
    div = f32.max_abs_divergence32(u, sp, ps)
    with _lib.options(INS_DISABLE_TEMP32_STAGE=1):
        _, su, stemp = run()
    print(geom, kind, gdir, diss, method, f"u {rell2(gu, st['u']):.2e} temp {rell2(gt, st['temp']):.2e} div {div * hmin / np.max(np.abs(st['u'])):.2e} "
          f"sequence: u {rell2(su, gu):.2e} temp {rell2(stemp, gt):.2e}")
    assert rell2(gu, st["u"]) < 5e-5 and rell2(gt, st["temp"]) < 5e-5
    assert div * hmin < 3e-5 * float(np.max(np.abs(st["u"])))
    assert rell2(su, gu) < 1e-5 and rell2(stemp, gt) < 1e-5


@pytest.mark.parametrize("geom,kind", [("mixed3d", "dirichlet"), ("wide3d", "any")])
def test_step_without_temp_is_the_isothermal_step(ins, oracle, geom, kind):
    """timestep32_ / timesteps32_ without `temp` on a setup that has a temperature equation: bit for bit the step of a setup without one."""
    from tests.test_gpu_parity import mirror

    o, f32 = oracle, ins.f32
    so, sp = _setups(ins, o, geom, kind, 1, True)
    plain = mirror(ins, so, o)
    g, D = so.grid, so.grid.D
    u0 = o.apply_bc_u(_r32(0.3 * fx.randn_field(g.N + (D,), 8)), 0.0, so)
    out = []
    for s in (sp, plain):
        ps = f32.default_psolver32(s)
        cache = f32.ERKCache32(ins.RKMethods.RK44(), s, ps)
        u = f32.to_f32(s, u0)
        assert f32.timestep32_(cache, u, 1e-3) is u
        f32.timesteps32_(cache, u, 1e-3, 2)
        out.append(u.cpu().numpy())
        del cache, ps
    assert np.array_equal(out[0], out[1])


def test_temperature_f32_refuses_what_it_does_not_cover(ins, oracle):
    o, f32 = oracle, ins.f32
    x = tuple(np.linspace(0.0, 1.0, 17) for _ in range(2))
    walls = ((ins.DirichletBC(), ins.DirichletBC()),) * 2
    # `temp` on a setup without a temperature equation
    plain = ins.Setup(x=x, boundary_conditions=walls, Re=100.0)
    ps = f32.psolver_wrap32(plain)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), plain, ps)
    with pytest.raises(ValueError):
        f32.timestep32_(cache, f32.vectorfield32(plain), 1e-3, temp=f32.scalarfield32(plain))
    with pytest.raises(ValueError):
        f32.timesteps32_(cache, f32.vectorfield32(plain), 1e-3, 2, temp=f32.scalarfield32(plain))
    # callable temperature boundary data
    hot = ins.DirichletBC(lambda x, y, t: 1.0 + 0 * x)
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (hot, ins.DirichletBC(0.0))), gdir=1)
    moving = ins.Setup(x=x, boundary_conditions=walls, temperature=T)
    with pytest.raises(NotImplementedError, match="constant boundary data"):
        f32.apply_bc_temp32_(f32.scalarfield32(moving), moving)
    ps = f32.psolver_wrap32(moving)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), moving, ps)
    with pytest.raises(NotImplementedError, match="constant boundary data"):
        f32.timestep32_(cache, f32.vectorfield32(moving), 1e-3, temp=f32.scalarfield32(moving))
    # a wall-bounded temperature run needs a wrapped solver: the only other Float32 solver names that route when it is asked for this grid, so no
    # stepper cache can reach the temperature loop without one
    T2 = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()),
                                                                                  (ins.DirichletBC(1.0), ins.DirichletBC(0.0))), gdir=1)
    sw = ins.Setup(x=x, boundary_conditions=walls, temperature=T2)
    with pytest.raises(Exception, match="ins_poisson_wrap_f32"):
        f32.psolver_spectral32(sw)
    # the native loop wants `temp` exactly when a descriptor is set
    from ins_amd import _lib

    ps = f32.psolver_wrap32(sw)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sw, ps)
    u, t = f32.vectorfield32(sw), f32.temperaturefield32(sw, lambda x, y: 0.5 + 0 * x * y)
    f32.timestep32_(cache, u, 1e-3, temp=t)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(t).all())
    lib = _lib.load()
    assert lib.ins_rk_step_ext_f32(cache._handle, 0.01, u.data_ptr(), None, 1e-3, None) == -1
    assert b"temperature" in lib.ins_last_error()


@pytest.fixture(scope="module")
def rb3d(ins):
    sys.path.insert(0, EX)
    spec = importlib.util.spec_from_file_location("RayleighBenard3D", os.path.join(EX, "RayleighBenard3D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {dtype: mod.main(n=12, tend=0.2, dt=1e-2, dtype=dtype, verbose=False) for dtype in ("float32", "float64")}


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_rayleigh_benard_3d(rb3d, dtype):
    """examples/RayleighBenard3D.py at n = 12, 20 steps: bounded temperature, heat enters at the hot plate and leaves at the cold one, solenoidal
    velocity at float32 level."""
    r = rb3d[dtype]
    lo, hi = r["nusselt"]
    print(dtype, f"Tmin {r['Tmin']:.6f} Tmax {r['Tmax']:.6f} Nu {lo:.4f} {hi:.4f} maxdiv*hmin/umax {r['maxdiv'] * r['hmin'] / r['umax']:.2e}")
    assert -1e-3 <= r["Tmin"] and r["Tmax"] <= 1 + 1e-3
    assert lo > 0 and hi > 0
    assert r["maxdiv"] * r["hmin"] < 3e-5 * r["umax"]


def test_rayleigh_benard_3d_float32_follows_float64(rb3d):
    """The three-step Float32 bound (5e-5) grown linearly over the 20 steps of a laminar start; the yardstick is the fp64 path."""
    err = rell2(rb3d["float32"]["temp"].astype(np.float64), rb3d["float64"]["temp"])
    print(f"rell2(temp32, temp64) = {err:.3e}")
    assert err < 20 * 5e-5 / 3
