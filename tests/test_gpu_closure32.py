"""The Smagorinsky closure and the steady body force of the `_f32` family (csrc/ins_smagforce32.hip, ins_smagforce_kernels.h; the extended Float32
stage loop of csrc/ins_f32.hip) against the oracle.  The checker is the one of tests/test_gpu_f32.py and tests/test_gpu_temperature32.py: the numpy
oracle in float64 on the float32-rounded inputs, `rell2` / `relmax`, the Float32 bounds of those files (2e-5 per operator, 5e-5 for three steps, 3e-5
for the scaled divergence).  The closure holds a square root of a sum of squares of differences; tools/closure32_emulate.py (the oracle chain with
metrics and inputs cast to numpy float32 against fp64, no GPU) gives at most 3.0e-7 for the stress and the closure force on every grid used here —
under a quarter of 2e-5, so the existing bounds stand."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from tests import fixtures as fx

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
THETA = 0.17
OP_TOL, STEP_TOL, DIV_TOL, SEQ_TOL = 2e-5, 5e-5, 3e-5, 1e-5


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


def _r32(a):
    return np.asfortranarray(np.asarray(a).astype(np.float32).astype(np.float64))


def _geom(o, name):
    from tests.test_gpu_f32 import _lid_setup, exact_box
    from tests.test_gpu_fields import _symmetric3d, _symuniform3d

    return {"dirichlet2d": fx.setup2d, "dirichlet3d": fx.setup3d, "mixed3d": fx.setup_mixed, "lid3d": _lid_setup,
            "periodic3d": lambda o: fx.setup_periodic(o, (12, 10, 8), D=3), "periodic2d": lambda o: fx.setup_periodic(o, (24, 18), D=2),
            "wide3d": lambda o: exact_box(o, (128, 16, 16)), "symmetric3d": _symmetric3d, "symuniform3d": _symuniform3d}[name](o)


def _sym_fields(sig, D):
    """the oracle's N + (D, D) stress as the D(D+1)/2 fields [xx, yy, (zz), xy, (xz, yz)]"""
    pairs = [(0, 0), (1, 1), (0, 1)] if D == 2 else [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    return np.stack([sig[..., a, b] for a, b in pairs], axis=-1)


# ------------------------------------------------------------------------------------------------------------------ 1. operators against the oracle
@pytest.mark.parametrize("geom", ["periodic2d", "periodic3d", "wide3d", "dirichlet3d", "mixed3d", "lid3d", "symmetric3d", "symuniform3d"])
def test_closure_operators_f32_match_oracle(ins, oracle, geom):
    from tests.test_gpu_parity import mirror

    o, f32 = oracle, ins.f32
    so = _geom(o, geom)
    sp = mirror(ins, so, o)
    g, D = so.grid, so.grid.D
    u_h = o.apply_bc_u(_r32(fx.randn_field(g.N + (D,), 1)), 0.0, so)
    u = f32.to_f32(sp, u_h)
    # smagtensor! (written on Ip)
    sig_h = o.smagtensor_(np.zeros(g.N + (D, D), order="F"), u_h, THETA, so)
    σ = f32.tensorfield32(sp)
    assert f32.smagtensor32_(σ, u, THETA, sp) is σ
    e_sig = relmax(σ.cpu().numpy().astype(np.float64), _sym_fields(sig_h, D))
    # the closure m(u, θ): the library's route for this grid
    m = f32.smagorinsky_closure32(sp)
    assert m._ins_closure == "smagorinsky" and m._ins_setup is sp
    s = m(u, THETA)
    assert s.dtype == torch.float32
    s_h = o.smagorinsky_closure(so)(u_h, THETA)
    e_s = relmax(s.cpu().numpy().astype(np.float64), s_h)
    # ... and the fp64 kernels as a second yardstick
    k64 = ins.to_numpy(ins.smagorinsky_closure(sp)(ins.from_numpy(sp, u_h), THETA))
    e_k = relmax(s.cpu().numpy().astype(np.float64), k64)
    print(geom, f"smagtensor {e_sig:.2e} closure {e_s:.2e} closure vs fp64 kernel {e_k:.2e}")
    assert np.max(np.abs(s_h)) > 0
    assert e_sig < OP_TOL and e_s < OP_TOL and e_k < OP_TOL


# ------------------------------------------------------------------------------------------------------------------ 2. one kernel against three kernels
def _walled(ins, case):
    Dr, Sy, Pe = ins.DirichletBC, ins.SymmetricBC, ins.PeriodicBC
    if case == "walls":
        x = (ins.tanh_grid(0.0, 1.0, 72, 1.2), ins.cosine_grid(0.0, 1.0, 12), ins.tanh_grid(0.0, 0.5, 10, 1.1))
        bc = ((Dr(), Dr((0.3, 0.0, 0.1))), (Dr(), Dr((1.0, 0.2, 0.0))), (Dr(), Dr()))
    elif case == "channel":
        x = (np.linspace(0.0, 2.0, 138), ins.tanh_grid(0.0, 1.0, 10, 1.5), ins.cosine_grid(0.0, 0.8, 9))
        bc = ((Pe(), Pe()), (Dr(), Dr()), (Sy(), Sy()))
    elif case == "mixed":
        x = (ins.cosine_grid(0.0, 1.0, 61), np.linspace(0.0, 0.7, 17), ins.tanh_grid(0.0, 1.3, 70, 1.3))
        bc = ((Sy(), Dr()), (Pe(), Pe()), (Dr(), Sy()))
    elif case == "outflow":
        Pr = ins.PressureBC
        x = (ins.tanh_grid(0.0, 2.0, 72, 1.2), ins.cosine_grid(0.0, 1.0, 12), np.linspace(0.0, 0.5, 11))
        bc = ((Dr((1.0, 0.0, 0.0)), Pr()), (Sy(), Sy()), (Dr(), Pr()))
    elif case == "symuniform":
        x = (np.linspace(0.0, 1.0, 71), np.linspace(0.0, 0.5, 13), np.linspace(0.0, 0.25, 11))
        bc = ((Sy(), Sy()), (Pe(), Pe()), (Sy(), Sy()))
    else:  # tiny
        x = (np.linspace(0.0, 1.0, 6), np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 7))
        bc = ((Dr(), Dr()), (Dr(), Sy()), (Sy(), Dr()))
    return ins.Setup(x=x, Re=1000.0, boundary_conditions=bc)


@pytest.mark.parametrize("case", [(64, 9, 4), (61, 16, 70), (5, 4, 6), (136, 20, 37), "walls", "channel", "mixed", "tiny", "symuniform", "outflow"])
def test_one_kernel_closure_force_f32_matches_the_three_kernel_sequence(ins, case):
    """The float instantiations of the one-kernel closure force (uniform periodic; GEN; GEN + STR) against k_smagtensor<float> -> k_bc_p<float> ->
    ins_divoftensor_f32 on the device, the z-chunk forced to 0 (default), 4, 8 and 32 planes: both are Float32 evaluations of one operator, each
    within the emulated 3e-7 of the exact result, so they agree inside the operator bound."""
    from ins_amd import _lib

    f32 = ins.f32
    if isinstance(case, tuple):
        sp = ins.Setup(x=tuple(np.linspace(0.0, L, ni + 1) for ni, L in zip(case, (1.0, 0.7, 1.3))), Re=1000.0)
        off = dict(INS_DISABLE_SMAGFORCE=1)
    else:
        sp = _walled(ins, case)
        off = dict(INS_DISABLE_SMAGFORCE_GEN=1)
    u = f32.apply_bc_u32_(f32.to_f32(sp, fx.randn_field(sp.grid.N + (3,), 5)), sp)
    m = f32.smagorinsky_closure32(sp)
    lib = _lib.load()
    assert lib.ins_smagorinsky_force_needs_sigma(sp.handle) == 0
    with _lib.options(**off):
        assert lib.ins_smagorinsky_force_needs_sigma(sp.handle) == 1
        three = m(u, THETA).cpu().numpy().astype(np.float64)
    assert np.max(np.abs(three)) > 0
    for zc in (0, 4, 8, 32):
        with _lib.options(INS_SMAGFORCE_ZC=zc):
            one = m(u, THETA).cpu().numpy().astype(np.float64)
        err = relmax(one, three)
        print(case, zc, f"{err:.2e}")
        assert err < OP_TOL, zc
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 3. three steps against the oracle
def _force(a, x, y, *zt):
    """Kolmogorov-type: sin(4πy) e_x, plus a weaker cos(2πx) e_y; steady"""
    return (a == 0) * np.sin(4 * np.pi * y) + (a == 1) * 0.3 * np.cos(2 * np.pi * x) + 0 * x * y + 0 * sum(zt[:-1], 0.0)


def _step_setups(ins, o, geom, closure, force, temp):
    """Oracle and product setups of `geom` with the chosen terms; the steady force field of the oracle is rounded to float32 like every input."""
    from tests.test_gpu_fields import mirror_temp, temp_bcs
    from tests.test_gpu_parity import mirror

    so0 = _geom(o, geom)
    D = so0.grid.D
    xin = [so0.grid.x[a][(2 if isinstance(so0.boundary_conditions[a][0], o.PressureBC) else 1):-1] for a in range(D)]
    T = None
    if temp:
        T = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=temp_bcs(o, so0, "dirichlet"), gdir=D - 1, dodissipation=True)
    Re = so0.Re if T is None else 1.0 / T.a1
    so = o.make_setup_ext(xin, so0.boundary_conditions, Re=Re, bodyforce=_force if force else None, issteadybodyforce=True, temperature=T)
    if force:
        so.bodyforce = _r32(so.bodyforce)
    base = mirror(ins, so0, o)
    sp = ins.Setup(x=xin, boundary_conditions=base.boundary_conditions, Re=Re, bodyforce=_force if force else None, issteadybodyforce=True)
    if temp:
        sp.temperature = mirror_temp(ins, o, T)
    if closure:
        so.closure_model = o.smagorinsky_closure(so)
        sp.closure_model = ins.f32.smagorinsky_closure32(sp) if closure == 32 else ins.smagorinsky_closure(sp)
    return so, sp


COMBOS = {"closure": (32, False, False), "force": (0, True, False), "closure+force": (64, True, False), "closure+force+temp": (32, True, True)}


@pytest.mark.parametrize("geom", ["periodic2d", "periodic3d", "wide3d", "mixed3d", "dirichlet2d"])
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("method", ["RK44", "Wray3"])
def test_closure_force_steps_f32_match_oracle(ins, oracle, geom, combo, method):
    """Three steps on the Float32 extended stage loop (timesteps32_ ×2 then timestep32_) against oracle.timestep_ext_ ×3 from the same
    float32-representable start.  `closure+force` hands the fp64-made library closure of the setup to the Float32 loop, the others the Float32-made."""
    o, f32 = oracle, ins.f32
    closure, force, temp = COMBOS[combo]
    so, sp = _step_setups(ins, o, geom, closure, force, temp)
    g, D = so.grid, so.grid.D
    pso = o.default_psolver(so)
    u0 = 0.5 * fx.randn_field(g.N + (D,), 31).astype(np.float32).astype(np.float64)
    u0 = o.apply_bc_u(o.project_(o.apply_bc_u(np.asfortranarray(u0), 0.0, so), so, pso, o.scalarfield(so)), 0.0, so)
    u0 = _r32(u0)
    t0 = _r32(o.apply_bc_temp(0.5 + 0.1 * fx.randn_field(g.N, 4), 0.0, so)) if temp else None
    dt = 0.3 * o.get_cfl_timestep(u0, so)
    θ = THETA if closure else None
    mo = getattr(o, method)()
    st = dict(setup=so, psolver=pso, u=u0.copy(order="F"), temp=None if t0 is None else t0.copy(order="F"), t=0.0, n=0)
    oc = o.ode_method_cache_ext(mo, so)
    for _ in range(3):
        st = o.timestep_ext_(mo, st, dt, oc, theta=θ)
    ps = f32.default_psolver32(sp)
    cache = f32.ERKCache32(getattr(ins.RKMethods, method)(), sp, ps)
    u = f32.to_f32(sp, u0)
    t = f32.to_f32(sp, t0) if temp else None
    f32.timesteps32_(cache, u, dt, 2, temp=t, θ=θ)
    r = f32.timestep32_(cache, u, dt, temp=t, θ=θ)
    assert (r[0] is u and r[1] is t) if temp else (r is u)
    gu = u.cpu().numpy().astype(np.float64)
    hmin = min(float(np.min(g.dx[a][1:-1])) for a in range(D))
    div = f32.max_abs_divergence32(u, sp, ps)
    eu = rell2(gu, st["u"])
    et = rell2(t.cpu().numpy().astype(np.float64), st["temp"]) if temp else 0.0
    print(geom, combo, method, f"u {eu:.2e} temp {et:.2e} div {div * hmin / np.max(np.abs(st['u'])):.2e}")
    assert eu < STEP_TOL and et < STEP_TOL
    assert div * hmin < DIV_TOL * float(np.max(np.abs(st["u"])))


# ------------------------------------------------------------------------------------------------------------------ 4. route identity
@pytest.mark.parametrize("geom", ["wide3d", "mixed3d"])
def test_no_closure_and_no_force_is_the_plain_step(ins, oracle, geom):
    """kind = 0 and a NULL force through the extended entry points: bit for bit the plain cache, chained steps included.  θ = 0 with a zero force
    field takes the extended route (another sequence of kernels) and agrees with the plain step to the sequence bound of the Float32 tests."""
    from ins_amd import _lib
    from tests.test_gpu_parity import mirror

    o, f32 = oracle, ins.f32
    so = _geom(o, geom)
    g, D = so.grid, so.grid.D
    u0 = o.apply_bc_u(_r32(0.3 * fx.randn_field(g.N + (D,), 8)), 0.0, so)
    lib = _lib.load()
    out = []
    for variant in ("plain", "kind0"):
        sp = mirror(ins, so, o)
        ps = f32.default_psolver32(sp)
        cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
        u = f32.to_f32(sp, u0)
        if variant == "plain":
            f32.timestep32_(cache, u, 1e-3)
            f32.timesteps32_(cache, u, 1e-3, 3)
        else:
            _lib.call("ins_rk_set_closure_f32", cache._handle, 0, 0.3)
            _lib.call("ins_rk_set_bodyforce_f32", cache._handle, None)
            _lib.check(lib.ins_rk_step_ext_f32(cache._handle, float(1.0 / sp.Re), u.data_ptr(), None, 1e-3, sp.stream))
            _lib.check(lib.ins_rk_steps_ext_f32(cache._handle, float(1.0 / sp.Re), u.data_ptr(), None, 1e-3, 3, sp.stream))
        out.append(u.cpu().numpy())
        del cache, ps
    assert np.array_equal(out[0], out[1])
    # θ = 0 and f = 0: the extended loop
    xin = [g.x[a][(2 if isinstance(so.boundary_conditions[a][0], o.PressureBC) else 1):-1] for a in range(D)]
    sp = ins.Setup(x=xin, boundary_conditions=mirror(ins, so, o).boundary_conditions, Re=so.Re, bodyforce=lambda a, x, y, z, t: 0 * (x + y + z),
                   issteadybodyforce=True)
    sp.closure_model = f32.smagorinsky_closure32(sp)
    ps = f32.default_psolver32(sp)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    u = f32.to_f32(sp, u0)
    f32.timestep32_(cache, u, 1e-3, θ=0.0)
    f32.timesteps32_(cache, u, 1e-3, 3, θ=0.0)
    err = rell2(u.cpu().numpy().astype(np.float64), out[0].astype(np.float64))
    print(geom, f"extended route with θ = 0, f = 0 against the plain step: {err:.2e}")
    assert err < SEQ_TOL


# ------------------------------------------------------------------------------------------------------------------ 5. the force is used
def test_steady_force_enters_the_step(ins, oracle):
    """u(Δt) with the force minus u(Δt) without it is Δt·f to first order for a solenoidal f (project! leaves it alone).  The remainder is the
    Δt²/2 term of the step, J·f with J the linearised momentum operator at u0; ‖J‖ <= 4 D ν / h² + 2 D max|u0| / h (diffusion and convection stencils),
    so the relative deviation from Δt·f is below Δt·‖J‖ / 2 — and below Δt·‖J‖, which the test asks.  Float32 rounding (1e-7 of |u| = 0.1 against
    Δt·|f| = 1e-3: 1e-5 relative) is far inside.  Before the force reached the Float32 loop this difference was exactly zero."""
    o, f32 = oracle, ins.f32
    n = (24, 18)
    x = tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n)
    fun = lambda a, x, y, t: (a == 0) * np.sin(4 * np.pi * y) + 0 * x  # noqa: E731
    so = o.make_setup(x, Re=1000.0)
    pso = o.default_psolver(so)
    u0 = 0.1 * fx.randn_field(so.grid.N + (2,), 3)
    u0 = _r32(o.apply_bc_u(o.project_(o.apply_bc_u(np.asfortranarray(u0), 0.0, so), so, pso, o.scalarfield(so)), 0.0, so))
    dt = 1e-3
    res = {}
    for name, bf in (("forced", fun), ("free", None)):
        sp = ins.Setup(x=x, Re=1000.0, bodyforce=bf, issteadybodyforce=True)
        ps = f32.psolver_spectral32(sp)
        cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
        u = f32.to_f32(sp, u0)
        f32.timestep32_(cache, u, dt)
        res[name] = u.cpu().numpy().astype(np.float64)
        if bf is not None:
            f = ins.to_numpy(sp.bodyforce)
        del cache, ps
    inner = (slice(1, -1), slice(1, -1))
    diff = (res["forced"] - res["free"])[inner]
    h = 1.0 / max(n)
    bound = dt * (4 * 2 * (1.0 / 1000.0) / h**2 + 2 * 2 * float(np.max(np.abs(u0))) / h)
    err = rell2(diff, dt * f[inner])
    print(f"(u_forced - u_free) against Δt f: {err:.3e} (first-order bound {bound:.3e})")
    assert np.max(np.abs(diff)) > 0
    assert err < bound < 0.1


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_closure32_refuses_what_it_does_not_cover(ins):
    from ins_amd import _lib

    f32 = ins.f32
    x = tuple(np.linspace(0.0, 1.0, 17) for _ in range(2))
    method = ins.RKMethods.RK44()

    def stepper(sp):
        ps = f32.psolver_spectral32(sp)
        return f32.ERKCache32(method, sp, ps), f32.vectorfield32(sp)

    # an unsteady body force
    sp = ins.Setup(x=x, Re=100.0, bodyforce=lambda a, xx, yy, t: np.sin(xx + t) * (a == 0) + 0 * yy, issteadybodyforce=False)
    cache, u = stepper(sp)
    for call in (lambda: f32.timestep32_(cache, u, 1e-3), lambda: f32.timesteps32_(cache, u, 1e-3, 2)):
        with pytest.raises(NotImplementedError, match="steady body force"):
            call()
    # a closure model that is not the library's; the library's closure of another setup
    sp = ins.Setup(x=x, Re=100.0)
    other = ins.Setup(x=x, Re=100.0)
    cache, u = stepper(sp)
    for m in (lambda u, θ: 0 * u, f32.smagorinsky_closure32(other)):
        sp.closure_model = m
        for call in (lambda: f32.timestep32_(cache, u, 1e-3, θ=THETA), lambda: f32.timesteps32_(cache, u, 1e-3, 2, θ=THETA)):
            with pytest.raises(NotImplementedError, match="ad32|fp64"):
                call()
    # the library's closure: a missing θ, a non-scalar θ
    for m in (f32.smagorinsky_closure32(sp), ins.smagorinsky_closure(sp)):
        sp.closure_model = m
        for θ in (None, torch.tensor(THETA), np.array([THETA, THETA])):
            for call in (lambda: f32.timestep32_(cache, u, 1e-3, θ=θ), lambda: f32.timesteps32_(cache, u, 1e-3, 2, θ=θ)):
                with pytest.raises(NotImplementedError, match="θ"):
                    call()
        f32.timestep32_(cache, u, 1e-3, θ=THETA)  # and with a scalar θ it runs
        assert bool(torch.isfinite(u).all())
    # slab (HALO) grids through the C entries
    xs = tuple(np.linspace(0.0, 1.0, n + 1) for n in (72, 12, 10))
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    slab = ins.Setup(x=xs, Re=1000.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    N = slab.grid.N
    u = torch.zeros(int(np.prod(N)) * 3, dtype=torch.float32, device=slab.device)
    σ = torch.zeros(int(np.prod(N)) * 6, dtype=torch.float32, device=slab.device)
    s = torch.zeros_like(u)
    lib = _lib.load()
    assert lib.ins_smagtensor_f32(slab.handle, THETA, u.data_ptr(), σ.data_ptr(), slab.stream) == -4
    assert b"slab" in lib.ins_last_error()
    assert lib.ins_smagorinsky_force_f32(slab.handle, THETA, u.data_ptr(), σ.data_ptr(), s.data_ptr(), slab.stream) == -4
    assert b"slab" in lib.ins_last_error()
    assert not bool(σ.any()) and not bool(s.any())


# ------------------------------------------------------------------------------------------------------------------ 7. example
def test_kolmogorov_2d_float32_follows_float64(ins):
    """examples/Kolmogorov2D.py at n = 32 for 20 steps: the three-step Float32 bound (5e-5) grown linearly over the 20 steps; the yardstick is the
    fp64 path.  The forcing feeds the flow in both."""
    sys.path.insert(0, EX)
    spec = importlib.util.spec_from_file_location("Kolmogorov2D", os.path.join(EX, "Kolmogorov2D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = {dtype: mod.main(n=32, tend=0.02, dt=1e-3, verbose=False, dtype=dtype) for dtype in ("float32", "float64")}
    err = rell2(r["float32"]["u"], r["float64"]["u"])
    E32 = [e for _, e in r["float32"]["energy"]]
    print(f"rell2(u32, u64) = {err:.3e}; E32 {E32[0]:.3e} -> {E32[-1]:.3e}")
    assert E32[-1] > E32[0] and r["float32"]["forced_mode"] > 0
    assert err < 20 * 5e-5 / 3
