"""The Float32 driver: `solve_unsteady` on float32 fields, the one-pass CFL time step, the float observers and the float spectrum
(csrc/ins_fields32.hip, csrc/ins_spectrum.hip, solver.py, processors.py).  References are the fp64 entries on the widened float32 input; bounds are
derived (CFL, interpolations), emulated on the CPU (tools/fields32_emulate.py: vorticity, Qfield) or taken from tests/test_gpu_f32.py (steps)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFL_TOL = 2.5e-7  # two float roundings (Δu to float, the division): 2 · 2⁻²³ ≈ 2.4e-7; the minimum is monotone
STEP_TOL = 5e-5   # tests/test_gpu_f32.py: a few Float32 RK steps against fp64, relative L2
DIV_TOL = 5e-5    # tests/test_gpu_f32.py: max|div u| · h against max|u| on the spectral Float32 solver


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def emu():
    return _load(os.path.join(ROOT, "tools", "fields32_emulate.py"), "fields32_emulate")


def rell2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b**2)), 1e-300))


def _mirror(ins, so, o):
    from tests.test_gpu_parity import mirror

    return mirror(ins, so, o)


def _cfl_grids(o):
    D, Pe, Pr, Sy = o.DirichletBC, o.PeriodicBC, o.PressureBC, o.SymmetricBC
    return {
        "walls2d": lambda: o.make_setup((o.tanh_grid(0.0, 2.0, 20, 1.2), o.cosine_grid(0.0, 1.0, 12)), ((Pe(), Pe()), (D(), D())), Re=1000.0),
        "periodic3d": lambda: o.make_setup(tuple(np.linspace(0.0, L, n + 1) for n, L in zip((70, 9, 5), (1.0, 0.7, 1.3))), Re=1000.0),
        "mixed3d": lambda: o.make_setup((o.tanh_grid(0.0, 5.0, 130), o.cosine_grid(0.0, 1.0, 34), o.tanh_grid(0.0, 0.8, 6)),
                                        ((Pe(), Pe()), (D(), Pr()), (Sy(), Sy())), Re=1000.0),
    }


# ------------------------------------------------------------------------------------------------------------------ 1. CFL
@pytest.mark.parametrize("geom", ["walls2d", "periodic3d", "mixed3d"])
def test_cfl_timestep32_against_fp64(ins, oracle, geom):
    """get_cfl_timestep32_ against get_cfl_timestep_ of the widened field: rows that cross a wavefront edge (70, 130 > 64 volumes), several rows per
    workgroup and several workgroup partials.  The minimum planted at the first and the last index of every Iu[α]; 1e6 in every volume outside
    Iu[α] without a ghost fill; a zero field."""
    f32 = ins.f32
    sp = _mirror(ins, _cfl_grids(oracle)[geom](), oracle)
    g = sp.grid
    D = g.dimension
    rng = np.random.default_rng(7)
    base = np.asfortranarray((0.5 + rng.random(g.N + (D,))) * rng.choice([-1.0, 1.0], g.N + (D,))).astype(np.float32)

    def both(h):
        u32 = f32.to_f32(sp, h)
        return f32.get_cfl_timestep32_(u32, sp), ins.get_cfl_timestep_(None, u32.double(), sp)

    got, want = both(base)
    print(f"{geom}: float {got:.9e} fp64 {want:.9e} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= CFL_TOL * want
    for a in range(D):
        assert all(hi > lo for lo, hi in g.Iu[a])
        for I in (tuple(lo for lo, _ in g.Iu[a]), tuple(hi - 1 for _, hi in g.Iu[a])):
            h = base.copy()
            h[I + (a,)] *= np.float32(1e3)
            got, want = both(h)
            planted = float(g.Δu[a][I[a]]) / abs(float(h[I + (a,)]))
            assert abs(want - planted) <= 1e-12 * planted, (a, I)  # the planted value is the minimum
            print(f"{geom} α={a} I={I}: float {got:.9e} fp64 {want:.9e} rel {abs(got - want) / want:.2e}")
            assert abs(got - want) <= CFL_TOL * want, (a, I)
    # adversarial: a huge velocity in every ghost volume and on every face outside Iu[α]; no ghost fill
    adv = np.full_like(base, 1e6)
    for a in range(D):
        sl = tuple(slice(lo, hi) for lo, hi in g.Iu[a]) + (a,)
        adv[sl] = base[sl]
    assert f32.get_cfl_timestep32_(f32.to_f32(sp, adv), sp) == f32.get_cfl_timestep32_(f32.to_f32(sp, base), sp)
    # zero field: the diffusive bound, formed in double and returned through the entry's float result
    bound = min(sp.Re * float(np.min(np.asarray(g.Δu[a])[g.Iu[a][a][0]:g.Iu[a][a][1]])) ** 2 / 2 for a in range(D))
    assert f32.get_cfl_timestep32_(f32.vectorfield32(sp), sp) == float(np.float32(bound))
    assert float(np.float32(ins.get_cfl_timestep_(None, ins.vectorfield(sp), sp))) == float(np.float32(bound))


# ------------------------------------------------------------------------------------------------------------------ 2. observers
@pytest.fixture(scope="module")
def observer_cases(ins, oracle, emu):
    """Per grid of tools/fields32_emulate.py: the setup, the float32 test field, the fp64 results of the four observers on it (computed once), and
    the emulated Float32 rounding errors."""
    out = {}
    for name, so in emu.grids(oracle).items():
        sp = _mirror(ins, so, oracle)
        h = emu.test_field(oracle, so)
        g = so.grid
        emulated = emu.emulate(h, g.N, g.Ip, g.dx, g.dxu)
        u32 = ins.f32.to_f32(sp, h)
        u64 = u32.double()
        D = sp.grid.dimension
        mk = (lambda: ins.scalarfield(sp)) if D == 2 else (lambda: ins.vectorfield(sp))
        ω = ins.vorticity_(mk(), u64, sp)
        ref = dict(ω=ω, up=ins.interpolate_u_p_(ins.vectorfield(sp), u64, sp), Q=ins.Qfield_(ins.scalarfield(sp), u64, sp))
        out[name] = dict(sp=sp, u32=u32, ref=ref, emulated=emulated)
    return out


def _relmax(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("name", ["walls2d 20x12", "mixed3d 34x20x6"])
def test_float_observers_against_fp64(ins, observer_cases, name):
    """vorticity32_ and Qfield32_ within 4 x the emulated Float32 rounding error of the fp64 entries on the same input, on the index ranges the kernels
    write; the two interpolations (one add, one halving) within 2⁻²⁴ of the sum of the magnitudes."""
    f32 = ins.f32
    c = observer_cases[name]
    sp, u32, ref, emulated = c["sp"], c["u32"], c["ref"], c["emulated"]
    g = sp.grid
    D = g.dimension
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    wbox = tuple(slice(0, n - 1) for n in g.N)
    mk = (lambda: f32.scalarfield32(sp)) if D == 2 else (lambda: f32.vectorfield32(sp))
    ω = f32.vorticity32_(mk(), u32, sp)
    eω = _relmax(ω[wbox], ref["ω"][wbox])
    Q = f32.Qfield32_(f32.scalarfield32(sp), u32, sp)
    eQ = _relmax(Q[ip], ref["Q"][ip])
    print(f"{name}: vorticity observed {eω:.3e} emulated {emulated['vorticity']:.3e}; Qfield observed {eQ:.3e} emulated {emulated['Qfield']:.3e}")
    assert eω <= 4 * emulated["vorticity"]
    assert eQ <= 4 * emulated["Qfield"]
    # interpolate_u_p: (u[I - e_α] + u[I]) / 2
    up = f32.interpolate_u_p32_(f32.vectorfield32(sp), u32, sp)
    u64 = u32.double()
    for a in range(D):
        lo = tuple(slice(l - (b == a), h - (b == a)) for b, (l, h) in enumerate(g.Ip))
        mag = u64[..., a][lo].abs() + u64[..., a][ip].abs()
        assert bool(((up[..., a][ip].double() - ref["up"][..., a][ip]).abs() <= 2.0**-24 * mag).all())
    # interpolate_ω_p of the float vorticity against the fp64 entry on the same (widened) input
    ω64 = ω.double()
    mk64 = (lambda: ins.scalarfield(sp)) if D == 2 else (lambda: ins.vectorfield(sp))
    ωp_ref = ins.interpolate_ω_p_(mk64(), ω64, sp)
    ωp = f32.interpolate_ω_p32_(mk(), ω, sp)
    comps = [(ω64, ωp, ωp_ref, (0, 1))] if D == 2 else [(ω64[..., a], ωp[..., a], ωp_ref[..., a], ((a + 1) % 3, (a + 2) % 3)) for a in range(3)]
    for w, got, want, dirs in comps:
        lo = tuple(slice(l - (b in dirs), h - (b in dirs)) for b, (l, h) in enumerate(g.Ip))
        mag = w[lo].abs() + w[ip].abs()
        assert bool(((got[ip].double() - want[ip]).abs() <= 2.0**-24 * mag).all())


# ------------------------------------------------------------------------------------------------------------------ 3. spectrum
# one box per transform route of ins_spectrum_create: the library plan in 2-D and in 3-D (32³: its y / z sides are not register-pass lengths; an odd
# box), the own passes on power-of-two sides, and on a 3 · 2^m side
SPECTRUM_BOXES = [(32, 32), (32, 32, 32), (20, 12, 10), (32, 128, 128), (96, 128, 96)]


@pytest.mark.parametrize("n", SPECTRUM_BOXES)
def test_spectrum_f32_is_the_fp64_spectrum_of_the_widened_field(ins, n):
    from ins_amd.processors import _Spectrum

    sp = ins.Setup(x=tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n), Re=1000.0)
    u32 = ins.f32.to_f32(sp, np.asfortranarray(np.random.default_rng(3).standard_normal(sp.grid.N + (len(n),))))
    spec = _Spectrum(sp, ins.spectral_stuff(sp)["inds"])
    got = spec(u32).clone()
    want = spec(u32.double()).clone()
    assert float(want.abs().max()) > 0
    assert torch.equal(got, want)
    # the processor's route
    a = ins.observespectrum(dict(u=u32, temp=None, t=0.0, n=0), setup=sp)["ehat"].value
    assert np.array_equal(a, want.cpu().numpy())
    del spec


# ------------------------------------------------------------------------------------------------------------------ 4. fixed Δt
def _tgv(a, x, y, z):
    s, c = np.sin, np.cos
    tp = 2 * np.pi
    return (a == 0) * s(tp * x) * c(tp * y) * c(tp * z) - (a == 1) * c(tp * x) * s(tp * y) * c(tp * z) + 0 * (a == 2) * z


@pytest.fixture(scope="module")
def tgv(ins):
    sp = ins.Setup(x=(np.linspace(0.0, 1.0, 33),) * 3, Re=1000.0)
    u64 = ins.velocityfield(sp, _tgv, 0.0, psolver=ins.psolver_spectral(sp))
    u32 = ins.f32.to_f32(sp, u64)
    return sp, u32


def test_fixed_dt_is_the_hand_loop_bit_for_bit(ins, tgv, monkeypatch):
    """solve_unsteady on float32 fields, RK44, 7 steps of a 32³ Taylor-Green vortex: one timesteps32_ without processors; with a fieldsaver every 3
    steps the calls 3, 3, 1 (the states at n = 3 and 6 are saved: a processor sees the states after a step, as on the fp64 path and in solver.jl:73-79);
    seven timestep32_ with INS_NO_PROCESSOR_BATCH; and within the Float32 step bound of the fp64 run."""
    f32 = ins.f32
    sp, u0 = tgv
    method, dt, nstep = ins.RKMethods.RK44(), 1e-3, 7
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(method, sp, ps)
    kw = dict(setup=sp, tlims=(0.0, nstep * dt), ustart=u0, method=method, psolver=ps, cache=cache, Δt=dt)
    (u, temp, t), out = ins.solve_unsteady(**kw)
    assert u.dtype == torch.float32 and temp is None and out == {} and u is not u0 and abs(t - nstep * dt) < 1e-15
    hand = f32.timesteps32_(cache, ins.copyfield(u0), nstep * dt / nstep, nstep)
    assert torch.equal(u, hand)
    # default solver and cache
    (ud, _, _), _ = ins.solve_unsteady(setup=sp, tlims=(0.0, nstep * dt), ustart=u0, method=method, Δt=dt)
    assert torch.equal(ud, hand)
    # a fieldsaver every 3 steps
    (us, _, _), out = ins.solve_unsteady(**kw, processors=dict(save=ins.fieldsaver(setup=sp, nupdate=3)))
    assert [s["n"] for s in out["save"]] == [3, 6]
    assert all(s["u"].dtype == np.float32 for s in out["save"])
    h = ins.copyfield(u0)
    step = nstep * dt / nstep
    f32.timesteps32_(cache, h, step, 3)
    assert np.array_equal(out["save"][0]["u"], ins.to_numpy(h))
    f32.timesteps32_(cache, h, step, 3)
    f32.timestep32_(cache, h, step)
    assert torch.equal(us, h)
    # one call per step
    monkeypatch.setenv("INS_NO_PROCESSOR_BATCH", "1")
    (u1, _, _), out = ins.solve_unsteady(**kw, processors=dict(save=ins.fieldsaver(setup=sp, nupdate=3)))
    monkeypatch.delenv("INS_NO_PROCESSOR_BATCH")
    h = ins.copyfield(u0)
    for _ in range(nstep):
        f32.timestep32_(cache, h, step)
    assert torch.equal(u1, h) and [s["n"] for s in out["save"]] == [3, 6]
    # against the fp64 driver
    (u64, _, _), _ = ins.solve_unsteady(setup=sp, tlims=(0.0, nstep * dt), ustart=u0.double(), method=method, Δt=dt)
    err = rell2(u.double().cpu().numpy(), u64.cpu().numpy())
    print(f"float32 against fp64 solve_unsteady, {nstep} steps: {err:.3e}")
    assert err < STEP_TOL
    del cache, ps


def test_fixed_dt_with_temperature_is_the_hand_loop(ins):
    """2-D Rayleigh-Bénard between walls, 16 x 16, on psolver_wrap32: (u, temp) of solve_unsteady equal the hand loop bit for bit."""
    f32 = ins.f32
    x = (np.linspace(0.0, 1.0, 17),) * 2
    walls = ((ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(), ins.DirichletBC()))
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()),
                                                                                 (ins.DirichletBC(1.0), ins.DirichletBC(0.0))), gdir=1)
    sp = ins.Setup(x=x, boundary_conditions=walls, temperature=T)
    ps = f32.psolver_wrap32(sp)
    method = ins.RKMethods.RK44()
    cache = f32.ERKCache32(method, sp, ps)
    u0 = f32.vectorfield32(sp)
    t0 = f32.temperaturefield32(sp, lambda x, y: 1.0 - y + 0.05 * np.sin(2 * np.pi * x) * np.sin(np.pi * y))
    dt = 1e-3
    (u, temp, t), out = ins.solve_unsteady(setup=sp, tlims=(0.0, 5 * dt), ustart=u0, tempstart=t0, method=method, psolver=ps, cache=cache, Δt=dt,
                                           processors=dict(save=ins.fieldsaver(setup=sp, nupdate=2)))
    assert [s["n"] for s in out["save"]] == [2, 4] and out["save"][0]["temp"].dtype == np.float32
    hu, ht = ins.copyfield(u0), ins.copyfield(t0)
    step = 5 * dt / 5
    for k in (2, 2):
        f32.timesteps32_(cache, hu, step, k, temp=ht)
    f32.timestep32_(cache, hu, step, temp=ht)
    assert float(u.abs().max()) > 0 and torch.equal(u, hu) and torch.equal(temp, ht)
    # the default solver of a wall-bounded grid is the wrapped one
    (ud, td, _), _ = ins.solve_unsteady(setup=sp, tlims=(0.0, 5 * dt), ustart=u0, tempstart=t0, method=method, Δt=dt)
    hu, ht = ins.copyfield(u0), ins.copyfield(t0)
    f32.timesteps32_(cache, hu, step, 5, temp=ht)
    assert torch.equal(ud, hu) and torch.equal(td, ht)
    with pytest.raises(ValueError):
        ins.solve_unsteady(setup=sp, tlims=(0.0, dt), ustart=u0, method=method, Δt=dt)  # a temperature equation without a temperature field
    del cache, ps


def test_fixed_dt_with_closure_and_body_force_is_the_hand_loop(ins):
    """2-D Kolmogorov flow 32², steady body force and the Smagorinsky closure with a scalar θ: equal to the hand loop bit for bit; θ = None refused."""
    f32 = ins.f32
    x = (np.linspace(0.0, 1.0, 33),) * 2
    sp = ins.Setup(x=x, Re=1000.0, bodyforce=lambda a, xx, yy, t: (a == 0) * np.sin(8 * np.pi * yy) + 0 * xx, issteadybodyforce=True)
    sp.closure_model = f32.smagorinsky_closure32(sp)
    method = ins.RKMethods.RK44()
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(method, sp, ps)
    u0 = f32.to_f32(sp, ins.random_field(sp, kp=4, seed=2, psolver=ins.psolver_spectral(sp)))
    dt, θ = 1e-3, 0.17
    (u, _, _), _ = ins.solve_unsteady(setup=sp, tlims=(0.0, 4 * dt), ustart=u0, method=method, psolver=ps, cache=cache, Δt=dt, θ=θ)
    hand = f32.timesteps32_(cache, ins.copyfield(u0), 4 * dt / 4, 4, θ=θ)
    assert torch.equal(u, hand)
    plain = ins.Setup(x=x, Re=1000.0)
    psp = f32.psolver_spectral32(plain)
    free = f32.timesteps32_(f32.ERKCache32(method, plain, psp), ins.copyfield(u0), 4 * dt / 4, 4)
    assert not torch.equal(free, hand)  # the force and the closure took part
    with pytest.raises(NotImplementedError):
        ins.solve_unsteady(setup=sp, tlims=(0.0, 4 * dt), ustart=u0, method=method, psolver=ps, cache=cache, Δt=dt)
    del cache, ps, psp


# ------------------------------------------------------------------------------------------------------------------ 5. adaptive Δt
def test_adaptive_dt_follows_the_cfl_step(ins):
    """16³ periodic, cfl = 0.9: every Δt taken is min(cfl · CFL step of the state before it, tend - t), recomputed in fp64 from the saved states;
    the run ends on tend exactly; n_adapt_Δt = 2 changes Δt on even n only; Δt_min is honoured."""
    f32 = ins.f32
    sp = ins.Setup(x=(np.linspace(0.0, 1.0, 17),) * 3, Re=1000.0)
    u0 = f32.to_f32(sp, ins.random_field(sp, kp=3, seed=1, psolver=ins.psolver_spectral(sp)))
    cfl = 0.9
    dt0 = cfl * ins.get_cfl_timestep_(None, u0.double(), sp)
    tend = 4.6 * dt0

    def run(**kw):
        (u, _, t), out = ins.solve_unsteady(setup=sp, tlims=(0.0, tend), ustart=u0, cfl=cfl, processors=dict(save=ins.fieldsaver(setup=sp)), **kw)
        states = [dict(u=ins.to_numpy(u0), t=0.0, n=0)] + out["save"]
        assert t == tend and states[-1]["t"] == tend and [s["n"] for s in states] == list(range(len(states)))
        assert bool(torch.isfinite(u).all())
        return states

    def cfl64(s):
        assert s["u"].dtype == np.float32
        return cfl * ins.get_cfl_timestep_(None, ins.from_numpy(sp, s["u"].astype(np.float64)), sp)

    states = run(n_adapt_Δt=1)
    assert 4 <= len(states) - 1 <= 8
    for a, b in zip(states[:-1], states[1:]):
        want = min(cfl64(a), tend - a["t"])
        got = b["t"] - a["t"]
        print(f"n = {a['n']}: Δt {got:.9e} want {want:.9e} rel {abs(got - want) / want:.2e}")
        assert abs(got - want) <= CFL_TOL * want + 4e-16 * tend  # (t is a running sum in double)
    states = run(n_adapt_Δt=2)
    for a, b in zip(states[:-1], states[1:]):
        got = b["t"] - a["t"]
        if a["n"] % 2 == 0:
            held = min(cfl64(a), tend - a["t"])
            assert abs(got - held) <= CFL_TOL * held + 4e-16 * tend
            held = cfl64(a)
        else:  # the step of the even n before it, clipped to tend
            want = min(held, tend - a["t"])
            assert abs(got - want) <= CFL_TOL * want + 4e-16 * tend
    dtmin = 1.5 * dt0
    states = run(Δt_min=dtmin)
    for a, b in zip(states[:-1], states[1:]):
        assert cfl64(a) < dtmin
        assert abs((b["t"] - a["t"]) - min(dtmin, tend - a["t"])) <= 4e-16 * tend


# ------------------------------------------------------------------------------------------------------------------ 6. processors
def test_processors_on_a_float32_state(ins, observer_cases, tmp_path):
    import base64

    f32 = ins.f32
    for name, c in observer_cases.items():
        sp, u32 = c["sp"], c["u32"]
        g = sp.grid
        D = g.dimension
        ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
        state = dict(u=ins.copyfield(u32), temp=None, t=0.25, n=0)
        mk = (lambda: f32.scalarfield32(sp)) if D == 2 else (lambda: f32.vectorfield32(sp))
        ub = f32.apply_bc_u32_(ins.copyfield(u32), sp)
        ωp = f32.interpolate_ω_p32_(mk(), f32.vorticity32_(mk(), ub, sp), sp)
        got = ins.observefield(state, setup=sp, fieldname="vorticity").value
        assert got.dtype == np.float32 and np.array_equal(got, ins.to_numpy(ωp[ip]))
        Q = f32.Qfield32_(f32.scalarfield32(sp), u32, sp)
        want = torch.log(torch.clamp(Q[ip], min=np.finfo(np.float64).eps))
        assert np.array_equal(ins.observefield(state, setup=sp, fieldname="Qfield").value, ins.to_numpy(want))
        up = f32.interpolate_u_p32_(f32.vectorfield32(sp), u32, sp)
        assert np.array_equal(ins.observefield(state, setup=sp, fieldname=1).value, ins.to_numpy(up[..., 1][ip]))
        for refused in ("pressure", "Dfield", "eig2field", "B1", "V2"):
            with pytest.raises(NotImplementedError, match="double"):
                ins.observefield(state, setup=sp, fieldname=refused)
        with pytest.raises(ValueError):
            ins.observefield(state, setup=sp, fieldname="nonsense")
        fn = ins.save_vtk(state, setup=sp, filename=str(tmp_path / f"s{D}"), fieldnames=("velocity", "vorticity"))
        import re

        m = re.search(r'Name="velocity" NumberOfComponents="3" format="binary">([^<]*)<', open(fn).read())
        raw = base64.b64decode(m.group(1))
        data = np.frombuffer(raw[8:], dtype=np.float64).reshape(-1, 3)
        host = ins.to_numpy(up[ip]).astype(np.float64)
        for a in range(D):
            assert np.array_equal(data[:, a], host[..., a].reshape(-1, order="F"))
    with pytest.raises(TypeError):
        ins.get_scale_numbers(u32, sp)


# ------------------------------------------------------------------------------------------------------------------ 7. example
def test_decaying_turbulence_example_in_float32(ins, tmp_path):
    ex = os.path.join(ROOT, "examples")
    sys.path.insert(0, ex)
    try:
        mod = _load(os.path.join(ex, "DecayingTurbulence3D.py"), "DecayingTurbulence3D_f32")
    finally:
        sys.path.remove(ex)
    n = 32
    r32 = mod.main(n=n, tend=0.01, kp=5, vtk=str(tmp_path), verbose=False, dtype="float32")
    r64 = mod.main(n=n, tend=0.01, kp=5, verbose=False)
    u = r32["u"]
    assert u.dtype == torch.float32 and bool(torch.isfinite(u).all()) and r32["t"] == 0.01
    print(f"max|div u| = {r32['maxdiv']:.3e}, max|u| = {float(u.abs().max()):.3e}")
    assert r32["maxdiv"] / n < DIV_TOL * float(u.abs().max())
    assert len(r32["ehat1"]) == len(r64["ehat1"]) and np.all(np.isfinite(r32["ehat1"]))
    assert r32["E1"] < r32["E0"]  # it decays
