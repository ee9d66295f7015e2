"""GPU: the Float32 pullbacks of the temperature equation (csrc/ins_temp_adjoint32.hip) and their `ins_amd.ad32` layer.

Every yardstick is existing code: the fp64 pullbacks (csrc/ins_temp_adjoint.hip), the existing Float32 forwards (gravity32_,
convection_diffusion_temp32_, dissipation32_, apply_bc_temp32_, timestep32_) and the fp64 `ad.timestep`.  The scheme is that of
tests/test_gpu_adjoint32.py: fields are random multiples of 2^-10 (float32-representable, and so are u + v and u - v) over the whole padded
array, ghosts included; dots and norms are taken in float64; every test prints `RATIO ...` lines before it asserts.

  1. transpose identities |<L v, w> - <v, L^T w>| / (|L v| |w|) with L the existing Float32 forward;
  2. value by value against the fp64 pullback on the same inputs promoted to double (max-norm, relative to max|result|);
  3. the fused per-stage entry against the sum of the operator-level entries, elementwise, and bitwise reproducibility;
  4. ad32.timestep with temperature: forward against timestep32_, gradients in u0 and temp0 against the fp64 ad.timestep; LMWray3; a closure;
  5. a Taylor test in temp0;  6. saved inputs are version-checked;  7. refusals;  8. examples/RayleighBenardGradient2D.py in Float32.

Bounds.  The ghost-fill pullback adds at most D ghost cotangents into a value: |r32 - r64| <= D 2^-24 sum|terms| elementwise.  A stencil
pullback is held to MARGIN = 4 x the error of the existing Float32 FORWARD of the same operator against its fp64 twin, measured in the same test
on the same geometry and inputs (the pullback gathers both product-rule branches, about twice the forward's products, and the maxima are taken
over different random fields).  The fused entry's tempbar is gravity^T + (dc/dtemp)^T and its ubar (dc/du)^T + dissipation^T: each is held to
4 x the larger of the two forward errors.  The fused entry adds at most four float parts, each addition rounding once:
|fused - sum parts| <= 4 2^-24 sum|parts| elementwise.

The dissipation pullback recomputes diffusion(u) and applies diffusion^T to wbar . u, a longer chain than its forward.  Emulated on the CPU
(tools/temp_adjoint32_emulate.py: the kernels' formulas in numpy float32, metrics and inputs cast to float32, against the same in float64; max-norm
relative, forward / pullback): setup2d 6.5e-8 / 8.6e-8, setup3d 8.8e-8 / 8.2e-8, mixed 1.1e-7 / 1.4e-7, periodic 12x10x8 9.3e-8 / 1.4e-7,
periodic 24x18 1.3e-7 / 7.4e-8, 70x66x4 1.1e-7 / 1.4e-7.  The pullback's error is at most 1.5 x the forward's, below the margin, so its bound
stays 4 x the forward yardstick.

Time steps: the gradient of J = 1/2 |u_N|^2 + 1/2 |temp_N|^2 with respect to the stacked start state (u0, temp0) is held, in relative L2 over the
stacked gradient, to 4 x the forward error of the stacked end state of the same run against fp64; the ad32 forward against timestep32_ to 4 x the
error of timestep32_ against fp64.
"""
import copy
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_adjoint32 import DT, EPS32, MARGIN, NSTEP, _u0, c32, defect, dot, mirror, nrm, pair, rell2, relmax
from tests.test_gpu_fields import mirror_temp, temp_bcs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def report(name, what, err, yard):
    """As tests/test_gpu_adjoint32.report; a yardstick of zero (gravity on a uniform grid: weights 1/2 and α2 = 1 are exact) prints no ratio."""
    print(f"RATIO {name} {what} err={err:.3e} yardstick={yard:.3e} ratio={err / yard if yard > 0 else float('nan'):.3f}")


def box70(o):
    """70 x 66 x 4 volumes, Dirichlet in x and y, periodic in z: a ragged second 64-wide tile, and 17 rows of 4-row tiles of the padded box over the
    8 bands of the banded launch (3 rows of tiles per band), so the sixth band is partly empty and the last two wholly."""
    x = (np.linspace(0.0, 7.0, 71), np.linspace(0.0, 6.6, 67), np.linspace(0.0, 0.4, 5))
    d = (o.DirichletBC(), o.DirichletBC())
    return o.make_setup(x, (d, d, (o.PeriodicBC(), o.PeriodicBC())), Re=1000.0)


GEOMS = {
    "setup2d": fx.setup2d,
    "setup3d": fx.setup3d,
    "mixed": fx.setup_mixed,
    "periodic3d": lambda o: fx.setup_periodic(o, (12, 10, 8), D=3),
    "periodic2d": lambda o: fx.setup_periodic(o, (24, 18), D=2),
    "box70": box70,
}
CASES = [("setup2d", "dirichlet"), ("setup2d", "symmetric"), ("setup3d", "dirichlet"), ("setup3d", "symmetric"), ("mixed", "dirichlet"),
         ("mixed", "symmetric"), ("periodic3d", "any"), ("periodic2d", "any"), ("box70", "dirichlet"), ("box70", "symmetric")]


def with_temperature(ins, o, name, kind, gdir, diss=True):
    so = GEOMS[name](o)
    T = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=temp_bcs(o, so, kind), dodissipation=diss, gdir=gdir)
    sp = mirror(ins, so, o)
    sp.temperature = mirror_temp(ins, o, T)
    return sp


def set_dissipation(ins, sp, diss):
    T = sp.temperature
    sp.temperature = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=T.boundary_conditions, dodissipation=diss, gdir=T.gdir)


def yardsticks(ins, sp, u, temp):
    """Errors of the existing Float32 forwards against their fp64 twins at (u, temp) = pairs of (float32, float64) fields (max-norm relative)."""
    F = ins.f32
    (u32, u64), (t32, t64) = u, temp
    Eg = relmax(F.gravity32_(F.vectorfield32(sp), t32, sp), ins.gravity_(ins.vectorfield(sp), t64, sp))
    Ec = relmax(F.convection_diffusion_temp32_(F.scalarfield32(sp), u32, t32, sp), ins.convection_diffusion_temp_(ins.scalarfield(sp), u64, t64, sp))
    Ed = relmax(F.dissipation32_(F.scalarfield32(sp), F.vectorfield32(sp), u32, sp), ins.dissipation_(ins.scalarfield(sp), ins.vectorfield(sp), u64, sp))
    return Eg, Ec, Ed


# ------------------------------------------------------------------------------------ 1. transpose identities
@pytest.mark.parametrize("name,kind", CASES)
def test_transpose_identities(ins, oracle, name, kind):
    D = GEOMS[name](oracle).grid.D
    for gdir in range(D):
        check_transpose_identities(ins, with_temperature(ins, oracle, name, kind, gdir), f"{name}/{kind}/gdir{gdir}")


def check_transpose_identities(ins, sp, label):
    F = ins.f32
    D = sp.grid.dimension
    u = pair(ins, sp, True, 1)
    v32, v64 = pair(ins, sp, True, 2)
    w32, w64 = pair(ins, sp, True, 3)
    temp = pair(ins, sp, False, 4)
    p32, p64 = pair(ins, sp, False, 5)
    q32, q64 = pair(ins, sp, False, 6)
    u32, t32 = u[0], temp[0]
    Eg, Ec, Ed = yardsticks(ins, sp, u, temp)
    zs, zv = (lambda: F.scalarfield32(sp)), (lambda: F.vectorfield32(sp))
    results = []
    # gravity: linear in temp
    results.append(("gravity_adjoint", defect(F.gravity32_(zv(), p32, sp), p64, w64, F.gravity_adjoint32_(zs(), w32, sp)), Eg))
    # convection_diffusion_temp is affine in temp at fixed u and in u at fixed temp: subtract the constant part
    Lp = F.convection_diffusion_temp32_(zs(), u32, p32, sp).double() - F.convection_diffusion_temp32_(zs(), u32, zs(), sp).double()
    _, tb = F.convection_diffusion_temp_adjoint32_(None, zs(), q32, u32, t32, sp)
    results.append(("convection_diffusion_temp_adjoint[temp]", defect(Lp, p64, q64, tb), Ec))
    Lv = F.convection_diffusion_temp32_(zs(), v32, t32, sp).double() - F.convection_diffusion_temp32_(zs(), zv(), t32, sp).double()
    ub, _ = F.convection_diffusion_temp_adjoint32_(zv(), None, q32, u32, t32, sp)
    results.append(("convection_diffusion_temp_adjoint[u]", defect(Lv, v64, q64, ub), Ec))
    # dissipation is quadratic: (f(u+v) - f(u-v))/2 = J(u) v, with u + v and u - v exact in float
    Jv = (F.dissipation32_(zs(), zv(), u32 + v32, sp).double() - F.dissipation32_(zs(), zv(), u32 - v32, sp).double()) / 2
    results.append(("dissipation_adjoint", defect(Jv, v64, q64, F.dissipation_adjoint32_(zv(), q32, u32, sp)), Ed))
    for what, err, yard in results:
        report(label, "transpose " + what, err, yard)
    # the affine ghost fill: L v = bc(v) - bc(0); the fill copies exactly, the pullback's float sums round: D 2^-24 <|v|, L^T|w|>
    Lb = F.apply_bc_temp32_(c32(ins, p32), sp) - F.apply_bc_temp32_(zs(), sp)
    LTq = F.apply_bc_temp_pullback32_(c32(ins, q32), sp)
    bound = D * EPS32 * dot(p64.abs(), ins.apply_bc_temp_pullback_(q64.abs(), 0.0, sp))
    db = abs(dot(Lb, q64) - dot(p64, LTq))
    print(f"RATIO {label} transpose apply_bc_temp defect={db:.3e} bound={bound:.3e}")
    assert nrm(Lb) > 0 and db <= bound
    for what, err, yard in results:
        assert err <= MARGIN * yard, (what, label, err, yard)


# ------------------------------------------------------------------------------------ 2. values against the fp64 twins
@pytest.mark.parametrize("name,kind", CASES)
def test_values_against_fp64(ins, oracle, name, kind):
    D = GEOMS[name](oracle).grid.D
    for gdir in range(D):
        check_values_against_fp64(ins, with_temperature(ins, oracle, name, kind, gdir), f"{name}/{kind}/gdir{gdir}")


def check_values_against_fp64(ins, sp, label):
    F = ins.f32
    D = sp.grid.dimension
    u = pair(ins, sp, True, 11)
    temp = pair(ins, sp, False, 12)
    (u32, u64), (t32, t64) = u, temp
    w32, w64 = pair(ins, sp, True, 13)
    q32, q64 = pair(ins, sp, False, 14)
    Eg, Ec, Ed = yardsticks(ins, sp, u, temp)
    zs, zv = (lambda: F.scalarfield32(sp)), (lambda: F.vectorfield32(sp))
    results = []
    results.append(("gravity_adjoint", relmax(F.gravity_adjoint32_(zs(), w32, sp), ins.gravity_adjoint_(ins.scalarfield(sp), w64, sp)), Eg))
    ub, tb = F.convection_diffusion_temp_adjoint32_(zv(), zs(), q32, u32, t32, sp)
    rub, rtb = ins.convection_diffusion_temp_adjoint_(ins.vectorfield(sp), ins.scalarfield(sp), q64, u64, t64, sp)
    results.append(("convection_diffusion_temp_adjoint[u]", relmax(ub, rub), Ec))
    results.append(("convection_diffusion_temp_adjoint[temp]", relmax(tb, rtb), Ec))
    ub1, _ = F.convection_diffusion_temp_adjoint32_(zv(), None, q32, u32, t32, sp)
    _, tb1 = F.convection_diffusion_temp_adjoint32_(None, zs(), q32, u32, t32, sp)
    results.append(("convection_diffusion_temp_adjoint[u alone]", relmax(ub1, rub), Ec))
    results.append(("convection_diffusion_temp_adjoint[temp alone]", relmax(tb1, rtb), Ec))
    results.append(("dissipation_adjoint", relmax(F.dissipation_adjoint32_(zv(), q32, u32, sp),
                                                  ins.dissipation_adjoint_(ins.vectorfield(sp), q64, u64, sp)), Ed))
    for diss in (True, False):
        set_dissipation(ins, sp, diss)
        junk = zs().fill_(7.0)  # tempbar is overwritten
        ub, tb = F.temperature_pullback32_(zv(), junk, w32, q32, u32, t32, sp)
        rub, rtb = ins.temperature_pullback_(ins.vectorfield(sp), ins.scalarfield(sp), w64, q64, u64, t64, sp)
        results.append((f"temperature_pullback[diss={diss}][temp]", relmax(tb, rtb), max(Eg, Ec)))
        results.append((f"temperature_pullback[diss={diss}][u]", relmax(ub, rub), max(Ec, Ed) if diss else Ec))
    for what, err, yard in results:
        report(label, "value " + what, err, yard)
    # ghost fill, elementwise: |r32 - r64| <= D 2^-24 sum|terms|, the sum of the terms' magnitudes being the fp64 pullback of |w|
    gb = (F.apply_bc_temp_pullback32_(c32(ins, q32), sp).double() - ins.apply_bc_temp_pullback_(ins.copyfield(q64), 0.0, sp)).abs()
    assert bool((gb <= D * EPS32 * ins.apply_bc_temp_pullback_(q64.abs(), 0.0, sp)).all())
    for what, err, yard in results:
        assert err <= MARGIN * yard, (what, label, err, yard)


# ------------------------------------------------------------------------------------ 3. fused against operator-level
@pytest.mark.parametrize("diss", [True, False])
@pytest.mark.parametrize("name,kind", CASES)
def test_fused_pullback_equals_the_operator_level_sum(ins, oracle, name, kind, diss):
    import torch

    F = ins.f32
    D = GEOMS[name](oracle).grid.D
    for gdir in range(D):
        sp = with_temperature(ins, oracle, name, kind, gdir, diss=diss)
        u32, _ = pair(ins, sp, True, 21)
        t32, _ = pair(ins, sp, False, 22)
        Fb32, _ = pair(ins, sp, True, 23)
        cb32, _ = pair(ins, sp, False, 24)
        zs, zv = (lambda: F.scalarfield32(sp)), (lambda: F.vectorfield32(sp))
        g = F.gravity_adjoint32_(zs(), Fb32, sp).double()
        cu, ct = F.convection_diffusion_temp_adjoint32_(zv(), zs(), cb32, u32, t32, sp)
        cu, ct = cu.double(), ct.double()
        d = F.dissipation_adjoint32_(zv(), cb32, u32, sp).double() if diss else torch.zeros_like(cu)
        ub, tb = F.temperature_pullback32_(zv(), zs().fill_(7.0), Fb32, cb32, u32, t32, sp)
        et = (tb.double() - (g + ct)).abs()
        eu = (ub.double() - (cu + d)).abs()
        bt, bu = 4 * EPS32 * (g.abs() + ct.abs()), 4 * EPS32 * (cu.abs() + d.abs())
        print(f"RATIO {name}/{kind}/gdir{gdir} diss={diss} fused-vs-parts temp max(err/bound)={float((et / bt.clamp_min(1e-300)).max()):.3f} "
              f"u max(err/bound)={float((eu / bu.clamp_min(1e-300)).max()):.3f}")
        assert float(tb.abs().max()) > 0 and float(ub.abs().max()) > 0
        assert bool((et <= bt).all()) and bool((eu <= bu).all())
        ub2, tb2 = F.temperature_pullback32_(zv(), zs().fill_(-3.0), Fb32, cb32, u32, t32, sp)
        assert torch.equal(ub, ub2) and torch.equal(tb, tb2)


# ------------------------------------------------------------------------------------ 4. ad32.timestep with temperature
def _rb_box(ins, closure_model=None):
    """16 x 8 tanh-grid Rayleigh-Benard box: plates Dirichlet 1 / 0, side walls symmetric, viscous heating on."""
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=1.0, dodissipation=True, gdir=1,
                                 boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0))))
    x = (ins.tanh_grid(0.0, 2.0, 16, 1.2), ins.tanh_grid(0.0, 1.0, 8, 1.2))
    walls = (ins.DirichletBC(), ins.DirichletBC())
    return ins.Setup(x=x, boundary_conditions=(walls, walls), temperature=T, closure_model=closure_model)


def _periodic_box(ins):
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, dodissipation=True, gdir=2, boundary_conditions=(per, per, per))
    sp = ins.Setup(x=tuple(np.linspace(0.0, 1.0, 9) for _ in range(3)), Re=1000.0)
    sp.temperature = T
    return sp


def _problem(ins, which, closure_model=None):
    """(setup, Float32 solver, fp64 solver)"""
    if which == "rb":
        sp = _rb_box(ins, closure_model)
        return sp, ins.f32.psolver_wrap32(sp, ins.psolver_direct(sp)), ins.psolver_direct(sp)
    sp = _periodic_box(ins)
    return sp, ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)


def _temp0(ins, sp, seed):
    """A ghost-filled start temperature, float32-representable, in both precisions."""
    _, r = pair(ins, sp, False, seed)
    t = ins.apply_bc_temp_(0.5 + 0.1 * r, 0.0, sp)
    t32 = ins.f32.to_f32(sp, t)
    t64 = ins.copyfield(t)
    t64.copy_(t32)
    return t32, t64


def _steps(ins, ad, method, sp, ps, u, temp, θ=None):
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u, temp=temp)
    for _ in range(NSTEP):
        st = ad.timestep(method, st, DT, θ=θ)
    return st.u, st.temp


def _J(u, temp):
    return 0.5 * (u.double() * u.double()).sum() + 0.5 * (temp.double() * temp.double()).sum()


def _stack(u, temp):
    import torch

    return torch.cat([u.detach().double().reshape(-1), temp.detach().double().reshape(-1)])


@pytest.mark.parametrize("which,method", [("rb", "RK44"), ("periodic", "RK44"), ("rb", "LMWray3")])
def test_timestep_forward_and_gradient(ins, which, method):
    import torch

    from ins_amd.time_steppers import _lmwray3_as_erk

    sp, ps32, ps64 = _problem(ins, which)
    m = ins.LMWray3() if method == "LMWray3" else ins.RKMethods.RK44()
    u32, u64 = _u0(ins, sp, ps64, 50)
    t32, t64 = _temp0(ins, sp, 51)
    # fp64: ad.timestep gives the reference forward and the reference gradient
    uu64, tt64 = u64.clone().requires_grad_(True), t64.clone().requires_grad_(True)
    ru, rt = _steps(ins, ins.ad, m, sp, ps64, uu64, tt64)
    gu64, gt64 = torch.autograd.grad(_J(ru, rt), (uu64, tt64))
    # the native Float32 step
    nu, nt = c32(ins, u32), c32(ins, t32)
    cache = ins.f32.ERKCache32(_lmwray3_as_erk(m) if method == "LMWray3" else m, sp, ps32)
    for _ in range(NSTEP):
        ins.f32.timestep32_(cache, nu, DT, temp=nt)
    yu, yt = rell2(nu, ru.detach()), rell2(nt, rt.detach())
    # ad32
    uu32, tt32 = u32.clone().requires_grad_(True), t32.clone().requires_grad_(True)
    ou, ot = _steps(ins, ins.ad32, m, sp, ps32, uu32, tt32)
    fu, ft = rell2(ou.detach(), nu), rell2(ot.detach(), nt)
    ref = _stack(ru, rt)
    yard = float((_stack(ou, ot) - ref).norm()) / float(ref.norm())
    print(f"RATIO {which}/{method} timestep forward ad32-vs-timestep32_ u={fu:.3e} temp={ft:.3e}; timestep32_-vs-fp64 u={yu:.3e} temp={yt:.3e}; "
          f"ad32-vs-fp64 stacked={yard:.3e}")
    gu32, gt32 = torch.autograd.grad(_J(ou, ot), (uu32, tt32))
    g64 = _stack(gu64, gt64)
    gerr = float((_stack(gu32, gt32) - g64).norm()) / float(g64.norm())
    report(f"{which}/{method}", "timestep gradient_(u0,temp0)", gerr, yard)
    print(f"RATIO {which}/{method} timestep gradient parts u0={rell2(gu32, gu64):.3e} temp0={rell2(gt32, gt64):.3e}")
    assert gu32.dtype == torch.float32 and gt32.dtype == torch.float32
    assert float(gu64.norm()) > 0 and float(gt64.norm()) > 0
    assert fu <= MARGIN * yu and ft <= MARGIN * yt, (fu, yu, ft, yt)
    assert gerr <= MARGIN * yard, (gerr, yard)


def test_timestep_closure_gradient(ins):
    """A torch closure m(u, θ) in float32 (neuralclosure.cnn cast to float; wrappedclosure takes periodic grids, so the periodic box): ∂J/∂θ
    against the fp64 ad.timestep of the same network in double."""
    import torch

    method = ins.RKMethods.RK44()
    sp64, _, ps64 = _problem(ins, "periodic")
    sp32, ps32, _ = _problem(ins, "periodic")
    net64 = ins.cnn(setup=sp64, radii=[1, 1], channels=[4, 3], activations=[torch.tanh, None], use_bias=[True, False], rng=7)
    net32 = copy.deepcopy(net64).float()
    with torch.no_grad():
        for a, b in zip(net64.parameters(), net32.parameters()):
            a.copy_(b)  # float32-representable weights in both
    sp32.closure_model = ins.wrappedclosure(net32, sp32)
    sp64.closure_model = ins.wrappedclosure(net64, sp64)
    u32, u64 = _u0(ins, sp64, ps64, 52)
    t32, t64 = _temp0(ins, sp64, 53)
    o32 = _steps(ins, ins.ad32, method, sp32, ps32, u32, t32)
    o64 = _steps(ins, ins.ad, method, sp64, ps64, u64, t64)
    ref = _stack(*o64)
    yard = float((_stack(*o32) - ref).norm()) / float(ref.norm())
    g32 = torch.autograd.grad(_J(*o32), list(net32.parameters()))
    g64 = torch.autograd.grad(_J(*o64), list(net64.parameters()))
    f32v = torch.cat([x.reshape(-1).double() for x in g32])
    f64v = torch.cat([x.reshape(-1) for x in g64])
    gerr = float((f32v - f64v).norm()) / float(f64v.norm())
    report("periodic/RK44", "timestep gradient_theta", gerr, yard)
    assert all(x.dtype == torch.float32 for x in g32)
    assert bool(torch.isfinite(f32v).all()) and float(f32v.norm()) > 0
    assert gerr <= MARGIN * yard, (gerr, yard)


# ------------------------------------------------------------------------------------ 5. Taylor test
def test_timestep_taylor_in_temp0(ins):
    """First-order Taylor remainder of J(temp0 + h v) in Float32, at step sizes whose second-order term is far above the rounding of J."""
    import torch

    method = ins.RKMethods.RK44()
    sp, ps32, ps64 = _problem(ins, "rb")
    u32, u64 = _u0(ins, sp, ps64, 54)
    t32, t64 = _temp0(ins, sp, 55)
    v32, _ = pair(ins, sp, False, 56)
    v32 = v32 * (float(t32.norm()) / float(v32.norm()))
    tt = t32.clone().requires_grad_(True)
    J0t = _J(*_steps(ins, ins.ad32, method, sp, ps32, u32, tt))
    (g,) = torch.autograd.grad(J0t, tt)
    J0, dJ = float(J0t.detach()), dot(g, v32)
    with torch.no_grad():
        noise = abs(J0 - float(_J(*_steps(ins, ins.ad, method, sp, ps64, u64, t64))))  # the forward rounding of J
        # J holds 1/2 |temp_N|^2, so the second-order term is about h^2 |v|^2 / 2 with |v| = |temp0|: 4e-2 .. 2.5e-3 of that part of J0;
        # the rounding of J is about 1e-7 of J0
        hs = [0.2, 0.1, 0.05]
        r = [abs(float(_J(*_steps(ins, ins.ad32, method, sp, ps32, u32, t32 + h * v32))) - J0 - h * dJ) for h in hs]
    ratios = [r[k] / r[k + 1] for k in range(2)]
    print(f"RATIO rb taylor J0={J0:.6e} dJ={dJ:.6e} noise={noise:.3e} remainders={r} ratios={ratios}")
    assert min(r) > 100 * noise, (r, noise)
    assert all(3.0 <= x <= 5.0 for x in ratios), (r, ratios)


# ------------------------------------------------------------------------------------ 6. version check
def test_saved_fields_are_version_checked(ins):
    """The fields a temperature backward reads go through save_for_backward: changing one in place before backward() raises."""
    import torch

    from ins_amd.autodiff32 import _StageRightHandSide

    sp, _, _ = _problem(ins, "periodic")
    ad = ins.ad32
    cases = [
        (lambda u, temp: ad.convection_diffusion_temp(u, temp, sp), "u"),
        (lambda u, temp: ad.convection_diffusion_temp(u, temp, sp), "temp"),
        (lambda u, temp: ad.dissipation(u, sp), "u"),
        (lambda u, temp: ad.momentum(u, temp, 0.0, sp), "u"),
        (lambda u, temp: sum(x.sum() for x in _StageRightHandSide.apply(u, temp, sp)), "u"),
        (lambda u, temp: sum(x.sum() for x in _StageRightHandSide.apply(u, temp, sp)), "temp"),
    ]
    for f, which in cases:
        u = pair(ins, sp, True, 60)[0].requires_grad_(True)
        temp = pair(ins, sp, False, 61)[0].requires_grad_(True)
        out = f(u, temp)
        with torch.no_grad():
            (u if which == "u" else temp).add_(1.0)
        with pytest.raises(RuntimeError):
            out.backward(torch.ones_like(out))
    # untouched, every one of them gives gradients
    u = pair(ins, sp, True, 60)[0].requires_grad_(True)
    temp = pair(ins, sp, False, 61)[0].requires_grad_(True)
    F, Ft = _StageRightHandSide.apply(u, temp, sp)
    gu, gt = torch.autograd.grad(F.sum() + Ft.sum(), (u, temp))
    assert gu.dtype == torch.float32 and float(gu.abs().max()) > 0 and float(gt.abs().max()) > 0


# ------------------------------------------------------------------------------------ 7. refusals
def test_refusals(ins):
    from ins_amd.time_steppers import _TempDesc

    F, ad = ins.f32, ins.ad32
    lib = ins._lib.load()
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)  # noqa: E731
    # callable temperature Dirichlet data
    x = tuple(np.linspace(0.0, 1.0, 17) for _ in range(2))
    walls = ((ins.DirichletBC(), ins.DirichletBC()),) * 2
    hot = ins.DirichletBC(lambda x, y, t: 1.0 + 0 * x)
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (hot, ins.DirichletBC(0.0))), gdir=1)
    moving = ins.Setup(x=x, boundary_conditions=walls, temperature=T)
    u, t = F.vectorfield32(moving), F.scalarfield32(moving)
    for call in (lambda: F.apply_bc_temp_pullback32_(t, moving), lambda: F.gravity_adjoint32_(t, u, moving),
                 lambda: F.convection_diffusion_temp_adjoint32_(F.vectorfield32(moving), F.scalarfield32(moving), t, u, t, moving),
                 lambda: F.dissipation_adjoint32_(F.vectorfield32(moving), t, u, moving),
                 lambda: F.temperature_pullback32_(F.vectorfield32(moving), F.scalarfield32(moving), u, t, u, t, moving),
                 lambda: ad.apply_bc_temp(t, 0.0, moving), lambda: ad.gravity(t, moving), lambda: ad.momentum(u, t, 0.0, moving)):
        with pytest.raises(NotImplementedError, match="constant boundary data"):
            call()
    method = ins.RKMethods.RK44()
    with pytest.raises(NotImplementedError, match="constant boundary data"):
        ad.timestep(method, ins.create_stepper(method, setup=moving, psolver=F.psolver_wrap32(moving), u=u, temp=t), 1e-3)
    # a slab grid: INS_ERR_UNSUPPORTED (-4) from each C entry, NotImplementedError from ad32
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    x3 = tuple(np.linspace(0.0, 1.0, 9) for _ in range(3))
    slab = ins.Setup(x=x3, Re=100.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    u, w, ub = F.vectorfield32(slab), F.vectorfield32(slab), F.vectorfield32(slab)
    t, q, tb = F.scalarfield32(slab), F.scalarfield32(slab), F.scalarfield32(slab)
    desc = _TempDesc(a2=1.0, a4=1e-3, diss_coef=0.1, gdir=2, dodissipation=1)
    codes = (C.c_int32 * 6)(*[ins.PeriodicBC().code] * 6)
    h, s = slab.handle, slab.stream
    assert lib.ins_apply_bc_temp_pullback_f32(h, codes, vp(tb), s) == -4
    assert b"slab" in lib.ins_last_error()
    assert lib.ins_gravity_adjoint_f32(h, 2, 1.0, vp(w), vp(tb), s) == -4
    assert lib.ins_convection_diffusion_temp_adjoint_f32(h, 1e-3, vp(u), vp(t), vp(q), vp(ub), vp(tb), s) == -4
    assert lib.ins_dissipation_adjoint_f32(h, 0.01, 0.1, vp(u), vp(q), vp(ub), s) == -4
    assert lib.ins_temperature_pullback_f32(h, C.byref(desc), 0.01, vp(u), vp(t), vp(w), vp(q), vp(ub), vp(tb), s) == -4
    for call in (lambda: ad.apply_bc_temp(t, 0.0, slab), lambda: ad.gravity(t, slab), lambda: ad.convection_diffusion_temp(u, t, slab),
                 lambda: ad.dissipation(u, slab), lambda: ad.momentum(u, t, 0.0, slab)):
        with pytest.raises(NotImplementedError):
            call()
    # in-place aliasing: INS_ERR_INVALID (-1)
    box = ins.Setup(x=x3, Re=100.0)
    u, w, ub = F.vectorfield32(box), F.vectorfield32(box), F.vectorfield32(box)
    t, q, tb = F.scalarfield32(box), F.scalarfield32(box), F.scalarfield32(box)
    h, s = box.handle, box.stream
    ncell = int(np.prod(box.grid.N))
    assert lib.ins_gravity_adjoint_f32(h, 2, 1.0, vp(w), vp(w, 2 * ncell), s) == -1
    assert lib.ins_gravity_adjoint_f32(h, 3, 1.0, vp(w), vp(tb), s) == -1  # gravity direction
    assert lib.ins_convection_diffusion_temp_adjoint_f32(h, 1e-3, vp(u), vp(t), vp(q), vp(ub), vp(q), s) == -1
    assert lib.ins_convection_diffusion_temp_adjoint_f32(h, 1e-3, vp(u), vp(t), vp(q), vp(ub), vp(t), s) == -1
    assert lib.ins_convection_diffusion_temp_adjoint_f32(h, 1e-3, vp(u), vp(t), vp(q), vp(u), vp(tb), s) == -1
    assert lib.ins_convection_diffusion_temp_adjoint_f32(h, 1e-3, vp(u), vp(t), vp(q), None, None, s) == -1
    assert lib.ins_dissipation_adjoint_f32(h, 0.01, 0.1, vp(u), vp(q), vp(u), s) == -1
    assert lib.ins_temperature_pullback_f32(h, C.byref(desc), 0.01, vp(u), vp(t), vp(w), vp(q), vp(u), vp(tb), s) == -1
    assert lib.ins_temperature_pullback_f32(h, C.byref(desc), 0.01, vp(u), vp(t), vp(w), vp(q), vp(w), vp(tb), s) == -1
    assert lib.ins_temperature_pullback_f32(h, C.byref(desc), 0.01, vp(u), vp(t), vp(w), vp(q), vp(ub), vp(t), s) == -1
    assert lib.ins_temperature_pullback_f32(h, C.byref(desc), 0.01, vp(u), vp(t), vp(w), vp(q), vp(ub), vp(q), s) == -1
    bad = (C.c_int32 * 6)(*[ins.PeriodicBC().code, ins.DirichletBC().code] * 3)
    assert lib.ins_apply_bc_temp_pullback_f32(h, bad, vp(tb), s) == -1  # periodic on one side only
    # a temperature field on a setup without a temperature equation
    with pytest.raises(NotImplementedError):
        ad.momentum(u, t, 0.0, box)
    with pytest.raises(ValueError):
        ad.gravity(t, box)


# ------------------------------------------------------------------------------------ 8. the example
def test_rayleigh_benard_gradient_example_float32(ins):
    """examples/RayleighBenardGradient2D.py with dtype=torch.float32 against its fp64 run: dJ = <grad, v> within the time-step bound —
    |<g32 - g64, v>| <= |g32 - g64| |v| <= MARGIN yard |g64| |v| with yard the forward error of the same run (the end temperature, which is all
    that Nu reads), plus 2^-24 |g64| |v| for the rounding of the direction v to float32."""
    import torch

    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("RayleighBenardGradient2D", os.path.join(ex, "RayleighBenardGradient2D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r32 = mod.main(n=16, nstep=5, dtype=torch.float32, verbose=False)
    r64 = mod.main(n=16, nstep=5, verbose=False)
    yard = rell2(r32["temp"], r64["temp"])
    scale = float(r64["grad"].norm()) * float(r64["v"].norm())
    gerr = rell2(r32["grad"], r64["grad"])
    print(f"RATIO example Nu32={r32['Nu']:.9e} Nu64={r64['Nu']:.9e} dJ32={r32['dJ']:.9e} dJ64={r64['dJ']:.9e} fd32={r32['fd']:.9e} "
          f"forward yardstick={yard:.3e} gradient rell2={gerr:.3e} |dJ32-dJ64|/(|g||v|)={abs(r32['dJ'] - r64['dJ']) / scale:.3e}")
    assert r32["grad"].dtype == torch.float32 and r32["ghost"] == 0.0
    assert np.isfinite(r32["Nu"]) and r32["Nu"] > 0
    assert gerr <= MARGIN * yard, (gerr, yard)
    assert abs(r32["dJ"] - r64["dJ"]) <= (MARGIN * yard + EPS32) * scale, (r32["dJ"], r64["dJ"], yard, scale)
