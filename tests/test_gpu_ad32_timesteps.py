"""GPU: `ad32.timesteps` and the native Float32 step pullbacks ins_rk_step_pullback_f32 / ins_rk_step_pullback_ext_f32 (csrc/ins_rk_adjoint_loop.h),
isothermal and with the temperature equation.

  1. forward: bitwise `f32.timesteps32_` with the same chunking, on a periodic box (spectral32) and on `mixed` (a wrapped direct solver);
  2. gradient.  There is no exact float reference, so both float routes are measured against fp64 on the widened inputs: g64 = the `ad.timesteps`
     gradient, e_native = |g32_native - g64| / |g64|, e_unrolled the same for 5 chained `ad32.timestep` calls.  Required:
     e_native <= MARGIN e_unrolled with MARGIN = 4 of tests/test_gpu_adjoint32.py: the native loop may order its sums differently, it must not be a
     worse transpose than the path users have today.  Both numbers are printed per case;
  3. transpose identity of one step in float: L a = (step(x + a) - step(x - a)) / 2 of the native Float32 step, the difference taken in fp64, on fields
     that are multiples of 2^-10 (x + a and x - a are exact), against Lᵀ b from the native pullback.  Δt = 1e-5 as in item 3 of
     tests/test_gpu_ad_timesteps.py, so that the step's cubic terms (Δt² / Δx² ~ 5e-9) stay under float rounding.  The defect
     |<L a, b> - <a, Lᵀ b>| / (|L a| |b|) is held to MARGIN x (s yard_project + yard_momentum): a step applies the projection s times at weight one
     and the momentum terms at weight Δt / Δx < 1, each with the error of the existing Float32 forward against its fp64 twin.  At this Δt the
     momentum, gravity and convection-diffusion pullbacks enter the step's Jacobian at about 1e-4, under the bound of 1e-6 to 4e-6 only by a
     factor of some tens: the item pins the ghost-fill and projection transposes and the loop's bookkeeping (a dropped or misplaced stage term is
     an error of order one), and would miss an error of a few percent in those pullbacks.  Item 2, at Δt = 1e-3 through 5 steps, carries that
     sensitivity;
  4. refusals, among them a wrapped spectral solver on a periodic box.
"""
import numpy as np
import pytest

from tests.test_gpu_ad_timesteps import DT, METHODS
from tests.test_gpu_adjoint32 import GEOMS, MARGIN, _u0, c32, defect, mirror, nrm, pair, rell2, yard_momentum, yard_project
from tests.test_gpu_temp_adjoint32 import CASES as TEMP_CASES
from tests.test_gpu_temp_adjoint32 import GEOMS as TEMP_GEOMS
from tests.test_gpu_temp_adjoint32 import _problem as temp_problem
from tests.test_gpu_temp_adjoint32 import _temp0, with_temperature

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_problems():
    """The problems are built once per module and released with it: solvers, reverse-step handles and native caches do not outlive the file."""
    import gc

    yield
    _cache.clear()
    gc.collect()


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def problem(ins, oracle, name):
    """(setup, Float32 solver, fp64 solver, (u32, u64), (t32, t64) or None, weights in fp64), built once per module.  `name`: a geometry of
    tests/test_gpu_adjoint32.GEOMS (isothermal; periodic boxes on the spectral solvers, the others on a wrapped direct one) or "temp:rb" /
    "temp:periodic" of tests/test_gpu_temp_adjoint32."""
    if name not in _cache:
        if isinstance(name, tuple):  # (geometry, kind of temperature sides, gdir, dissipation) of tests/test_gpu_temp_adjoint32.with_temperature
            sp = with_temperature(ins, oracle, *name)
            if name[0].startswith("periodic"):
                ps32, ps64 = ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)
            else:
                ps64 = ins.psolver_direct(sp)
                ps32 = ins.f32.psolver_wrap32(sp, ins.psolver_direct(sp))
            temp = _temp0(ins, sp, 51)
        elif name.startswith("temp:"):
            sp, ps32, ps64 = temp_problem(ins, name[5:])
            temp = _temp0(ins, sp, 51)
        else:
            sp = mirror(ins, GEOMS[name](oracle), oracle)
            if name.startswith("periodic"):
                ps32, ps64 = ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)
            else:
                ps64 = ins.psolver_direct(sp)
                ps32 = ins.f32.psolver_wrap32(sp, ins.psolver_direct(sp))
            temp = None
        u = _u0(ins, sp, ps64, 50)
        w = pair(ins, sp, True, 52)[1].abs()
        wt = pair(ins, sp, False, 53)[1].abs()
        _cache[name] = (sp, ps32, ps64, u, temp, (w, wt))
    return _cache[name]


def loss(u, temp, w):
    out = 0.5 * (w[0] * u.double() * u.double()).sum()
    return out if temp is None else out + 0.5 * (w[1] * temp.double() * temp.double()).sum()


def stack(gs):
    import torch

    return torch.cat([g.detach().double().reshape(-1) for g in gs])


def gradient(ins, ad, rollout, method, sp, ps, u, temp, w, nsteps, every):
    import torch

    xs = [u.clone().requires_grad_(True)] + ([] if temp is None else [temp.clone().requires_grad_(True)])
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=xs[0], temp=None if temp is None else xs[1])
    if rollout:
        st = ad.timesteps(method, st, DT, nsteps, checkpoint_every=every)
    else:
        for _ in range(nsteps):
            st = ad.timestep(method, st, DT)
    gs = torch.autograd.grad(loss(st.u, st.temp, w), xs)
    assert all(g.dtype == x.dtype for g, x in zip(gs, xs))
    return stack(gs)


# ------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name", ["periodic32_2d", "mixed", "temp:rb", "temp:periodic"])
def test_forward_is_the_native_loop(ins, oracle, name):
    import torch

    sp, ps32, _, (u32, _), temp, _ = problem(ins, oracle, name)
    t32 = None if temp is None else temp[0]
    method = ins.RKMethods.RK44()
    ubefore = u32.clone()
    uu = u32.clone().requires_grad_(True)
    tt = None if t32 is None else t32.clone().requires_grad_(True)
    got = ins.ad32.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps32, u=uu, temp=tt), DT, 5, checkpoint_every=2)
    assert got.u.grad_fn is not None and got.u.dtype == torch.float32 and got.n == 5 and abs(got.t - 5 * DT) < 1e-15
    assert torch.equal(uu.detach(), ubefore), "the input was changed"
    cache = ins.f32.ERKCache32(method, sp, ps32)
    nu, nt = c32(ins, u32), None if t32 is None else c32(ins, t32)
    for n in (2, 2, 1):
        ins.f32.timesteps32_(cache, nu, DT, n, temp=nt)
    assert torch.equal(got.u.detach(), nu), "not bitwise the native loop with the same chunking"
    if t32 is not None:
        assert got.temp.grad_fn is not None and torch.equal(got.temp.detach(), nt) and torch.equal(tt.detach(), t32)
    with torch.no_grad():
        a = ins.ad32.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps32, u=uu, temp=tt), DT, 5, checkpoint_every=2)
    assert a.u.grad_fn is None and not a.u.requires_grad
    one = c32(ins, u32)
    ins.f32.timesteps32_(cache, one, DT, 5, temp=None if t32 is None else c32(ins, t32))
    assert torch.equal(a.u, one), "without grad: not the one native call"


# ------------------------------------------------------------------------------------ 2. gradient against fp64, native against unrolled
def check_gradient(ins, oracle, name, mname, nsteps, every):
    sp, ps32, ps64, (u32, u64), temp, w = problem(ins, oracle, name)
    t32, t64 = (None, None) if temp is None else temp
    method = METHODS[mname](ins)
    key = ("g", name, mname, nsteps)
    if key not in _cache:
        g64 = gradient(ins, ins.ad, True, method, sp, ps64, u64, t64, w, nsteps, None)
        gun = gradient(ins, ins.ad32, False, method, sp, ps32, u32, t32, w, nsteps, None)
        _cache[key] = (g64, float((gun - g64).norm()) / float(g64.norm()))
    g64, e_unrolled = _cache[key]
    gnat = gradient(ins, ins.ad32, True, method, sp, ps32, u32, t32, w, nsteps, every)
    e_native = float((gnat - g64).norm()) / float(g64.norm())
    print(f"RATIO ad32.timesteps {name} {mname} nsteps={nsteps} every={every}: e_native={e_native:.3e} e_unrolled={e_unrolled:.3e} "
          f"ratio={e_native / e_unrolled:.3f}")
    assert float(g64.norm()) > 0 and e_unrolled > 0
    assert e_native <= MARGIN * e_unrolled, (name, mname, nsteps, every, e_native, e_unrolled)


@pytest.mark.parametrize("name", ["periodic32_2d", "periodic32_3d", "box_dirichlet", "mixed", "temp:rb", "temp:periodic"])
def test_gradient_geometries(ins, oracle, name):
    check_gradient(ins, oracle, name, "RK44", 5, 2)


@pytest.mark.parametrize("diss", [True, False])
@pytest.mark.parametrize("name,kind", [c for c in TEMP_CASES if c[0] != "box70"])
def test_gradient_temperature_spread(ins, oracle, name, kind, diss):
    """The coupled Float32 loop over the geometries, kinds of temperature sides (Dirichlet; symmetric / pressure; periodic), gravity directions and
    dissipation on and off of tests/test_gpu_temp_adjoint32.py: periodic boxes on the spectral solvers, the others on a wrapped direct one."""
    D = TEMP_GEOMS[name](oracle).grid.D
    for gdir in sorted({1, D - 1}):
        check_gradient(ins, oracle, (name, kind, gdir, diss), "RK44", 5, 2)


def test_periodic_box_with_a_wrapped_solver_is_refused(ins, oracle):
    """The 7 x 7 periodic box has an odd number of volumes, so only a wrapped direct solver serves it.  There the existing native forward
    `timesteps32_` does not refill the ghost volumes between the wrapped projections of a step: after 5 RK44 steps it is 2.0e-3 from the fp64 loop,
    where `ad32.timestep` is 1.0e-7 from it (measured), and a gradient taken along that rollout measured e_native = 1.8e-3 against
    e_unrolled = 1.5e-7.  The forward kernels are not this feature's to change, so `ad32.timesteps` refuses the configuration and names the
    routes that work."""
    sp, ps32, _, (u32, _), _, _ = problem(ins, oracle, "box_periodic")
    method = ins.RKMethods.RK44()
    with pytest.raises(NotImplementedError, match="timestep step by step"):
        ins.ad32.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps32, u=u32.clone().requires_grad_(True)), DT, 5, checkpoint_every=2)


@pytest.mark.parametrize("mname", ["RK33C2", "LMWray3", "DOPRI6"])
@pytest.mark.parametrize("name", ["box_dirichlet", "temp:rb"])
def test_gradient_methods(ins, oracle, name, mname):
    check_gradient(ins, oracle, name, mname, 5, 2)


@pytest.mark.parametrize("nsteps,every", [(1, 1), (5, 1), (5, 5), (3, None)])
@pytest.mark.parametrize("name", ["mixed", "temp:rb"])
def test_gradient_chunkings(ins, oracle, name, nsteps, every):
    check_gradient(ins, oracle, name, "RK44", nsteps, every)


def test_gradient_with_steady_body_force(ins, oracle):
    """The force is in the forward and in the recomputation of the stage inputs."""
    so = GEOMS["box_dirichlet"](oracle)
    bcs = tuple((ins.DirichletBC(), ins.DirichletBC()) for _ in range(2))
    sp = ins.Setup(x=tuple(so.grid.x[a][1:-1] for a in range(2)), boundary_conditions=bcs, Re=so.Re,
                   bodyforce=lambda a, x, y, t: (3.0 * np.sin(2 * np.pi * y) + 0 * x) if a == 0 else (2.0 * np.cos(2 * np.pi * x) + 0 * y), issteadybodyforce=True)
    ps64 = ins.psolver_direct(sp)
    ps32 = ins.f32.psolver_wrap32(sp, ins.psolver_direct(sp))
    u32, u64 = _u0(ins, sp, ps64, 54)
    w = (pair(ins, sp, True, 55)[1].abs(), None)
    method = ins.RKMethods.RK44()
    g64 = gradient(ins, ins.ad, True, method, sp, ps64, u64, None, w, 5, 2)
    e_unrolled = float((gradient(ins, ins.ad32, False, method, sp, ps32, u32, None, w, 5, None) - g64).norm()) / float(g64.norm())
    e_native = float((gradient(ins, ins.ad32, True, method, sp, ps32, u32, None, w, 5, 2) - g64).norm()) / float(g64.norm())
    print(f"RATIO ad32.timesteps steady body force: e_native={e_native:.3e} e_unrolled={e_unrolled:.3e}")
    assert e_native <= MARGIN * e_unrolled, (e_native, e_unrolled)


# ------------------------------------------------------------------------------------ 3. transpose identity of one step
@pytest.mark.parametrize("name", ["box_dirichlet", "periodic32_2d", "temp:rb"])
def test_step_transpose_identity(ins, oracle, name):
    sp, ps32, ps64, _, temp, _ = problem(ins, oracle, name)
    F = ins.f32
    method = ins.RKMethods.RK44()
    dt = 1e-5
    cache = F.ERKCache32(method, sp, ps32)
    adj = ins.ad32._step_adjoint(method, sp, ps32)
    coupled = temp is not None
    x, a, b = [[pair(ins, sp, True, seed)[0]] + ([pair(ins, sp, False, seed + 1)[0]] if coupled else []) for seed in (60, 62, 64)]

    def step(fields):
        u = c32(ins, fields[0])
        t = c32(ins, fields[1]) if coupled else None
        F.timestep32_(cache, u, dt, temp=t)
        return stack([u] + ([t] if coupled else []))

    La = (step([p + q for p, q in zip(x, a)]) - step([p - q for p, q in zip(x, a)])) / 2
    bars = [c32(ins, f) for f in b]
    adj.step_pullback_(bars[0], x[0], dt, *((bars[1], x[1]) if coupled else ()))
    err = defect(La, stack(a), stack(b), stack(bars))
    yard = len(method.b) * yard_project(ins, sp, ps32, ps64) + yard_momentum(ins, sp)
    print(f"RATIO ad32 step transpose {name}: defect={err:.3e} yardstick={yard:.3e} ratio={err / yard:.3f}")
    assert nrm(La) > 0 and err <= MARGIN * yard, (err, yard)


# ------------------------------------------------------------------------------------ 4. refusals
def test_refusals(ins):
    F = ins.f32
    x = (np.linspace(0.0, 1.0, 17), np.linspace(0.0, 1.0, 17))
    method = ins.RKMethods.RK44()
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    walls = ((ins.DirichletBC(), ins.DirichletBC()),) * 2
    lid = (ins.DirichletBC(), ins.DirichletBC(lambda a, x, y, t: (1.0 + 0 * x) if a == 0 else 0 * x))
    hot = ins.DirichletBC(lambda x, y, t: 1.0 + 0 * x)
    Tper = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per), gdir=1)
    Thot = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (hot, ins.DirichletBC(0.0))), gdir=1)

    def run(sp, ps=None, temp=False, u=None):
        ps = F.default_psolver32(sp) if ps is None else ps
        u = F.vectorfield32(sp).requires_grad_(True) if u is None else u
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=u, temp=F.scalarfield32(sp) if temp else None)
        return ins.ad32.timesteps(method, st, DT, 2)

    plain = ins.Setup(x=x, Re=100.0)
    run(plain)  # the plain setup runs
    refused = [
        (ins.Setup(x=x, Re=100.0, closure_model=lambda u, θ: θ * u), False),
        (ins.Setup(x=x, Re=100.0, temperature=Tper), False),  # a temperature equation without stepper.temp
        (ins.Setup(x=x, Re=100.0, boundary_conditions=(per, lid)), False),
        (ins.Setup(x=x, boundary_conditions=walls, temperature=Thot), True),
        (ins.Setup(x=x, Re=100.0, bodyforce=lambda a, x, y, t: np.sin(t) + 0 * x + 0 * y, issteadybodyforce=False), False),
    ]
    for sp, temp in refused:
        with pytest.raises(NotImplementedError, match="timestep "):
            run(sp, temp=temp)
    # a wrapped spectral solver on a periodic box: from ad32, and from the C entry at create time (INS_ERR_UNSUPPORTED = -4)
    wrapped = F.psolver_wrap32(plain, ins.psolver_spectral(plain))
    with pytest.raises(NotImplementedError, match="psolver_wrap32 around psolver_spectral"):
        run(plain, ps=wrapped)
    with pytest.raises(RuntimeError, match="wrapped spectral solver"):
        ins.ad32._OPS.rk_adjoint_create(method, plain, wrapped)
    # mixed precisions
    with pytest.raises(TypeError, match=r"ad\.timesteps"):
        run(plain, u=ins.vectorfield(plain))
    with pytest.raises(TypeError, match="psolver"):
        run(plain, ps=ins.psolver_spectral(plain))
    with pytest.raises(TypeError, match=r"ad32\.timesteps"):
        st = ins.create_stepper(method, setup=plain, psolver=ins.psolver_spectral(plain), u=F.vectorfield32(plain))
        ins.ad.timesteps(method, st, DT, 2)
    with pytest.raises(ValueError, match="needs setup.temperature"):
        run(plain, temp=True)
    # aliasing: INS_ERR_INVALID (-1)
    lib = ins._lib.load()
    adj = ins.ad32._step_adjoint(method, plain, F.default_psolver32(plain))
    u = F.vectorfield32(plain)
    p = F._ptr(plain, u, 2)
    assert lib.ins_rk_step_pullback_f32(adj._handle, 0.01, p, None, 1e-3, p, plain.stream) == -1 and b"alias" in lib.ins_last_error()
