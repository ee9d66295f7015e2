"""GPU: the pullbacks of the temperature equation (csrc/ins_temp_adjoint.hip) and their `ins_amd.ad` layer.

  1. transpose identities |<L v, w> - <v, L^T w>| <= tol |L v| |w| over the whole padded arrays: the linear part of apply_bc_temp, gravity,
     convection_diffusion_temp in temp and in u; dissipation is quadratic in u, so (f(u+v) - f(u-v))/2 = J(u) v exactly (tol 1e-11: sums of
     large terms of both signs, as tests/test_gpu_fields.py);
  2. value by value against the dense transposes of the CPU oracle's forward operators (unit probes).  The oracle's own central differences
     reproduce its linearisations to rounding on all five ORACLE_GEOMS (convection_diffusion_temp affine in u: <= 2.7e-16 relative, dissipation
     quadratic: <= 6.4e-16, the largest on `mixed`), checked on the CPU, so no geometry needs another bound;
  3. the fused per-stage entry against the sum of the four operator-level entries, bitwise reproducibility, 256^3 and 96^3 boxes;
  4. torch.autograd.gradcheck of the four `ad` functions and of ad.momentum(u, temp, ...);
  5. ad.timestep with temperature against the native extended stage loop;
  6. Taylor tests through 20 RK44 steps of a 64^2 Rayleigh-Benard box (temp0, u0, closure parameters);
  7. saved inputs are version-checked;
  8. examples/RayleighBenardGradient2D.py.
"""
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_adjoint import GEOMS, ORACLE_GEOMS, TOL, _periodic_box, _randn_field, _taylor, _u0, check_transpose, dot, mirror, rand, relmax
from tests.test_gpu_fields import mirror_temp, temp_bcs

pytestmark = pytest.mark.gpu

DISS_TOL = 1e-11  # tests/test_gpu_fields.py:112
KINDS = ["dirichlet", "function", "any"]


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def with_temperature(ins, o, name, kind, gdir, dodissipation=True):
    """(oracle setup, mirrored GPU setup) of GEOMS[name] with temperature BCs built like test_gpu_fields.temp_bcs."""
    so = GEOMS[name](o)
    so.temperature = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=temp_bcs(o, so, kind), dodissipation=dodissipation, gdir=gdir)
    sp = mirror(ins, so, o)
    sp.temperature = mirror_temp(ins, o, so.temperature)
    return so, sp


def gdirs(o, name):
    D = GEOMS[name](o).grid.D
    return sorted({1, D - 1})


def trel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------ 1. transpose identities
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(GEOMS))
def test_transpose_identities(ins, oracle, name, kind):
    for gdir in gdirs(oracle, name):
        _, sp = with_temperature(ins, oracle, name, kind, gdir)
        check_transpose_identities(ins, sp)


def check_transpose_identities(ins, sp):
    """The transpose identities of every temperature pullback on one setup with a temperature equation."""
    u, v, w = rand(ins, sp, True, 1), rand(ins, sp, True, 2), rand(ins, sp, True, 3)
    temp, p, q = rand(ins, sp, False, 4), rand(ins, sp, False, 5), rand(ins, sp, False, 6)
    zs, zv = ins.scalarfield(sp), ins.vectorfield(sp)
    # ghost fill: L p = bc(p) - bc(0)
    Lp = ins.apply_bc_temp(p, 0.3, sp) - ins.apply_bc_temp(zs, 0.3, sp)
    check_transpose(Lp, p, q, ins.apply_bc_temp_pullback_(ins.copyfield(q), 0.3, sp))
    # gravity: temp -> u
    check_transpose(ins.gravity(p, sp), p, w, ins.gravity_adjoint_(ins.scalarfield(sp), w, sp))
    # convection_diffusion_temp in temp at fixed u, and in u at fixed temp (affine in each: the constant part removed)
    Lt = ins.convection_diffusion_temp(u, p, sp) - ins.convection_diffusion_temp(u, zs, sp)
    check_transpose(Lt, p, q, ins.convection_diffusion_temp_adjoint_(None, ins.scalarfield(sp), q, u, temp, sp)[1])
    Lu = ins.convection_diffusion_temp(v, temp, sp) - ins.convection_diffusion_temp(zv, temp, sp)
    check_transpose(Lu, v, q, ins.convection_diffusion_temp_adjoint_(ins.vectorfield(sp), None, q, u, temp, sp)[0])
    # both halves in one call give the same two results
    ub, tb = ins.convection_diffusion_temp_adjoint_(ins.vectorfield(sp), ins.scalarfield(sp), q, u, temp, sp)
    check_transpose(Lu, v, q, ub)
    check_transpose(Lt, p, q, tb)
    # dissipation: quadratic in u
    Jv = (ins.dissipation(u + v, sp) - ins.dissipation(u - v, sp)) / 2
    check_transpose(Jv, v, q, ins.dissipation_adjoint_(ins.vectorfield(sp), q, u, sp), tol=DISS_TOL)


# ------------------------------------------------------------------------------------ 2. against the oracle, value by value
def dense_transpose_apply(L, shape, w):
    """(dL)^T w of a linear map L on numpy fields of `shape`, by unit probes."""
    n = int(np.prod(shape))
    wf = w.reshape(-1, order="F")
    out = np.empty(n)
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        out[k] = np.dot(wf, L(e.reshape(shape, order="F")).reshape(-1, order="F"))
        e[k] = 0.0
    return out.reshape(shape, order="F")


@pytest.mark.parametrize("name", ORACLE_GEOMS)
def test_pullbacks_match_oracle_transposes(ins, oracle, name):
    o = oracle
    for gdir in gdirs(o, name):
        for kind in KINDS if gdir == 1 else KINDS[:1]:
            so, sp = with_temperature(ins, o, name, kind, gdir)
            N, D = tuple(so.grid.N), so.grid.D
            vs, ss = N + (D,), N
            u, temp = fx.randn_field(vs, 20), fx.randn_field(ss, 23)
            w, q = fx.randn_field(vs, 21), fx.randn_field(ss, 22)
            ug, tg, wg, qg = (ins.from_numpy(sp, x) for x in (u, temp, w, q))
            zs = np.zeros(ss, order="F")
            cases = [("apply_bc_temp", lambda x: o.apply_bc_temp(x, 0.3, so) - o.apply_bc_temp(zs, 0.3, so), ss, q,
                      ins.apply_bc_temp_pullback_(ins.copyfield(qg), 0.3, sp), TOL)]
            if kind == KINDS[0]:  # the boundary kinds enter the ghost fill only
                ub, tb = ins.convection_diffusion_temp_adjoint_(ins.vectorfield(sp), ins.scalarfield(sp), qg, ug, tg, sp)
                c0 = o.convection_diffusion_temp(u, zs, so)
                cases += [
                    ("gravity", lambda x: o.gravity(x, so), ss, w, ins.gravity_adjoint_(ins.scalarfield(sp), wg, sp), TOL),
                    ("convection_diffusion_temp/temp", lambda x: o.convection_diffusion_temp(u, x, so) - c0, ss, q, tb, TOL),
                    ("convection_diffusion_temp/u",
                     lambda x: (o.convection_diffusion_temp(u + x, temp, so) - o.convection_diffusion_temp(u - x, temp, so)) / 2, vs, q, ub, TOL),
                ]
                if gdir == 1:  # no gravity direction in it
                    cases.append(("dissipation", lambda x: (o.dissipation(u + x, so) - o.dissipation(u - x, so)) / 2, vs, q,
                                  ins.dissipation_adjoint_(ins.vectorfield(sp), qg, ug, sp), DISS_TOL))
            for what, L, shape, cot, got, tol in cases:
                ref = dense_transpose_apply(L, shape, cot)
                err = relmax(ins.to_numpy(got), ref)
                print(f"{name} {kind} gdir={gdir} {what}: {err:.2e}")
                assert err <= tol, (what, kind, gdir, err)


# ------------------------------------------------------------------------------------ 3. fused against operator-level
def _fused_and_sum(ins, sp, u, temp, Fbar, cbar, base):
    """temperature_pullback_ on top of `base` (what momentum_pullback_ wrote) and the same from the four operator-level entries."""
    import torch

    junk = torch.full_like(cbar, 7.0)  # tempbar is overwritten
    ub, tb = ins.temperature_pullback_(ins.copyfield(base), junk, Fbar, cbar, u, temp, sp)
    rub, rtb = ins.copyfield(base), torch.zeros_like(cbar)
    ins.gravity_adjoint_(rtb, Fbar, sp)
    ins.convection_diffusion_temp_adjoint_(rub, rtb, cbar, u, temp, sp)
    if sp.temperature.dodissipation:
        ins.dissipation_adjoint_(rub, cbar, u, sp)
    return ub, tb, rub, rtb


@pytest.mark.parametrize("diss", [True, False])
@pytest.mark.parametrize("name", list(GEOMS))
def test_fused_pullback_equals_the_operator_level_sum(ins, oracle, name, diss):
    import torch

    for gdir in gdirs(oracle, name):
        _, sp = with_temperature(ins, oracle, name, "dirichlet", gdir, dodissipation=diss)
        check_fused_pullback(ins, sp)
    torch.cuda.synchronize()


def check_fused_pullback(ins, sp):
    """temperature_pullback_ against the sum of the operator-level entries, on zeros and on top of a momentum pullback; bitwise reproducible."""
    import torch

    u, Fbar = rand(ins, sp, True, 7), rand(ins, sp, True, 8)
    temp, cbar = rand(ins, sp, False, 9), rand(ins, sp, False, 10)
    for base in (ins.vectorfield(sp), ins.momentum_pullback_(ins.vectorfield(sp), Fbar, u, sp)):
        ub, tb, rub, rtb = _fused_and_sum(ins, sp, u, temp, Fbar, cbar, base)
        assert trel(ub, rub) <= TOL and trel(tb, rtb) <= TOL, (trel(ub, rub), trel(tb, rtb))
        ub2, tb2, _, _ = _fused_and_sum(ins, sp, u, temp, Fbar, cbar, base)
        assert torch.equal(ub, ub2) and torch.equal(tb, tb2)


def _scalar_randn(ins, sp, seed):
    import torch

    f = ins.scalarfield(sp)
    g = torch.Generator(device=sp.device).manual_seed(seed)
    f.copy_(torch.randn(f.shape, generator=g, dtype=torch.float64, device=sp.device))
    return f


@pytest.mark.parametrize("n", [256, 96])
def test_fused_pullback_on_large_periodic_boxes(ins, n):
    import torch

    sp = _periodic_box(ins, n)
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    for diss in (True, False):
        sp.temperature = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per, per), dodissipation=diss, gdir=2)
        u, Fbar = _randn_field(ins, sp, 70), _randn_field(ins, sp, 71)
        temp, cbar = _scalar_randn(ins, sp, 72), _scalar_randn(ins, sp, 73)
        base = ins.momentum_pullback_(ins.vectorfield(sp), Fbar, u, sp)
        ub, tb, rub, rtb = _fused_and_sum(ins, sp, u, temp, Fbar, cbar, base)
        assert trel(ub, rub) <= TOL and trel(tb, rtb) <= TOL, (trel(ub, rub), trel(tb, rtb))
        del rub, rtb
        ub2, tb2 = ins.temperature_pullback_(ins.copyfield(base), torch.zeros_like(cbar), Fbar, cbar, u, temp, sp)
        assert torch.equal(ub, ub2) and torch.equal(tb, tb2)
        del ub, tb, ub2, tb2, base, u, Fbar, temp, cbar
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------ 4. torch.autograd.gradcheck
@pytest.mark.parametrize("kind", ["PeriodicBC", "DirichletBC"])
def test_gradcheck_temperature_functions(ins, oracle, kind):
    import torch

    o = oracle
    x = (np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9))
    bc = getattr(o, kind)()
    so = o.make_setup(x, ((bc, bc), (bc, bc)), Re=100.0)
    so.temperature = o.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=temp_bcs(o, so, "dirichlet"), gdir=1)
    sp = mirror(ins, so, o)
    sp.temperature = mirror_temp(ins, o, so.temperature)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6)
    u = rand(ins, sp, True, 30).requires_grad_(True)
    temp = rand(ins, sp, False, 31).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda tt: ins.ad.apply_bc_temp(tt, 0.3, sp), (temp,), **kw)
    assert torch.autograd.gradcheck(lambda tt: ins.ad.gravity(tt, sp), (temp,), **kw)
    assert torch.autograd.gradcheck(lambda uu, tt: ins.ad.convection_diffusion_temp(uu, tt, sp), (u, temp), **kw)
    assert torch.autograd.gradcheck(lambda uu: ins.ad.dissipation(uu, sp), (u,), **kw)
    assert torch.autograd.gradcheck(lambda uu, tt: ins.ad.momentum(uu, tt, 0.0, sp), (u, temp), **kw)
    # forward values are those of the allocating twins
    with torch.no_grad():
        assert trel(ins.ad.momentum(u, temp, 0.0, sp), ins.momentum(u.detach(), temp.detach(), 0.0, sp)) <= TOL
        assert trel(ins.ad.dissipation(u, sp), ins.dissipation(u.detach(), sp)) <= TOL


# ------------------------------------------------------------------------------------ 5. ad.timestep forward = native step
def _rb_setup(ins, n, closure_model=None, square=True):
    """Wall-bounded Rayleigh-Benard box: tanh grid, hot bottom plate T = 1, cold top plate T = 0, insulated side walls (examples/RayleighBenard2D.py)."""
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=1.0, dodissipation=True, gdir=1,
                                 boundary_conditions=((ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0))))
    x = (ins.tanh_grid(0.0, 1.0 if square else 2.0, n if square else 2 * n, 1.2), ins.tanh_grid(0.0, 1.0, n, 1.2))
    walls = (ins.DirichletBC(), ins.DirichletBC())
    return ins.Setup(x=x, boundary_conditions=(walls, walls), temperature=T, closure_model=closure_model)


def _rb_temp0(ins, sp):
    return ins.temperaturefield(sp, lambda x, y: 0.5 + np.maximum(np.sin(20 * np.pi * x) / 100, 0) + 0 * y)


@pytest.mark.parametrize("name,method", [("periodic32_3d", "RK44"), ("mixed", "RK44"), ("rb2d", "RK44"), ("rb2d", "Wray3"), ("mixed", "Wray3")])
def test_ad_timestep_forward_matches_native(ins, oracle, name, method):
    import torch

    if name == "rb2d":
        sp = _rb_setup(ins, 16, square=False)
    else:
        _, sp = with_temperature(ins, oracle, name, "dirichlet", GEOMS[name](oracle).grid.D - 1)
    ps = ins.default_psolver(sp)
    m = getattr(ins.RKMethods, method)()
    u0 = _u0(ins, sp, ps, 40)
    t0 = ins.apply_bc_temp(0.5 + 0.1 * rand(ins, sp, False, 41), 0.0, sp)
    dt = 1e-3
    ref = ins.timestep(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u0, temp=t0), dt)
    with torch.no_grad():
        got = ins.ad.timestep(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u0, temp=t0), dt)
    eu, et = trel(got.u, ref.u), trel(got.temp, ref.temp)
    print(f"{name} {method}: u {eu:.2e}, temp {et:.2e}")
    assert eu <= TOL and et <= TOL, (eu, et)
    assert got.t == pytest.approx(ref.t) and got.n == ref.n


# ------------------------------------------------------------------------------------ 6. Taylor tests through 20 RK44 steps
# 64^2 Rayleigh-Benard box, Δt = 2e-3, J = the final lower-plate Nusselt number.  ε0 was chosen with the CPU oracle (oracle.timestep_ext_ on the same box,
# fields and directions, dJ from a central difference at ε0/1000): its own remainders at ε0, ε0/2, ε0/4, ε0/8 quarter with ratios
#   temp0: ε0 = 0.1 -> 4.000, 4.000, 4.000   (ε0 = 1: 4.004, 4.002, 4.001)
#   u0:    ε0 = 0.1 -> 4.005, 4.001, 4.000   (ε0 = 1: 4.197, 4.102, 4.029)
#   θ:     ε0 = 0.2 -> 4.005, 4.003, 4.001   (ε0 = 1: 4.025, 4.013, 4.006)
# with remainders between 6e-5 and 0.4 (temp0, u0) and 8e-8 and 5e-6 (θ), far above the rounding of J ≈ 45.
RB_N, RB_STEPS, RB_DT = 64, 20, 2e-3


def _nusselt(ins, sp, temp):
    import torch

    g = sp.grid
    dx = torch.as_tensor(np.asarray(g.Δ[0], dtype=np.float64), device=sp.device)
    return ((-(temp[:, 1] - temp[:, 0]) / float(g.Δu[1][0])) * dx)[1:-1].sum()


def _final_nusselt(ins, sp, ps, u0, temp0, θ=None):
    method = ins.RKMethods.RK44()
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u0, temp=temp0)
    for _ in range(RB_STEPS):
        st = ins.ad.timestep(method, st, RB_DT, θ=θ)
    return _nusselt(ins, sp, st.temp)


def _rb_problem(ins, closure_model=None):
    sp = _rb_setup(ins, RB_N, closure_model)
    ps = ins.default_psolver(sp)
    return sp, ps, 0.1 * _u0(ins, sp, ps, 50), _rb_temp0(ins, sp)


def _check_gradient(J, dJ, eps0, e):
    _taylor(J, dJ, eps0)
    fd = (J(e) - J(-e)) / (2 * e)
    print(f"dJ = {dJ:.12e}, central difference {fd:.12e}, relative {abs(fd - dJ) / abs(dJ):.2e}")
    assert abs(fd - dJ) <= 1e-6 * abs(dJ), (fd, dJ)


def test_nusselt_gradient_wrt_temp0(ins):
    import torch

    sp, ps, u0, temp0 = _rb_problem(ins)
    v = rand(ins, sp, False, 51)
    tt = temp0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_final_nusselt(ins, sp, ps, u0, tt), tt)

    def J(e):
        with torch.no_grad():
            return float(_final_nusselt(ins, sp, ps, u0, temp0 + e * v))

    _check_gradient(J, dot(g, v), 0.1, 1e-3)


def test_nusselt_gradient_wrt_u0(ins):
    import torch

    sp, ps, u0, temp0 = _rb_problem(ins)
    v = _u0(ins, sp, ps, 52)
    uu = u0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_final_nusselt(ins, sp, ps, uu, temp0), uu)

    def J(e):
        with torch.no_grad():
            return float(_final_nusselt(ins, sp, ps, u0 + e * v, temp0))

    _check_gradient(J, dot(g, v), 0.1, 1e-4)


def test_nusselt_gradient_wrt_closure_parameters(ins):
    """a-posteriori training on Rayleigh-Benard data: a torch closure m(u, θ) with the temperature equation on."""
    import torch

    def m(u, θ):
        return θ[0] * u + θ[1] * u * u

    sp, ps, u0, temp0 = _rb_problem(ins, m)
    θ0 = torch.tensor([-0.5, 0.2], dtype=torch.float64, device=sp.device)
    dθ = torch.tensor([0.7, -0.3], dtype=torch.float64, device=sp.device)
    th = θ0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_final_nusselt(ins, sp, ps, u0, temp0, th), th)

    def J(e):
        with torch.no_grad():
            return float(_final_nusselt(ins, sp, ps, u0, temp0, θ0 + e * dθ))

    _check_gradient(J, float((g * dθ).sum()), 0.2, 1e-3)


# ------------------------------------------------------------------------------------ 7. version check
def test_saved_fields_are_version_checked(ins):
    """The fields a temperature backward reads go through save_for_backward: changing one in place before backward() raises."""
    import torch

    sp = _periodic_box(ins, 32)
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    sp.temperature = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per, per), gdir=2)
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()

    def step(u, temp):
        st = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u, temp=temp), 1e-3)
        return st.u.sum() + st.temp.sum()

    cases = [
        (lambda u, temp: ins.ad.convection_diffusion_temp(u, temp, sp), "u"),
        (lambda u, temp: ins.ad.convection_diffusion_temp(u, temp, sp), "temp"),
        (lambda u, temp: ins.ad.dissipation(u, sp), "u"),
        (lambda u, temp: ins.ad.momentum(u, temp, 0.0, sp), "u"),
    ]
    for f, which in cases:
        u = _randn_field(ins, sp, 64).requires_grad_(True)
        temp = _scalar_randn(ins, sp, 65).requires_grad_(True)
        out = f(u, temp)
        with torch.no_grad():
            (u if which == "u" else temp).add_(1.0)
        with pytest.raises(RuntimeError):
            out.backward(torch.ones_like(out))
    # the per-stage right-hand side of ad.timestep saves the ghost-filled fields it made itself; its inputs are what the first ghost fill copies,
    # so the Function that reads them directly is exercised here
    from ins_amd.autodiff import _StageRightHandSide

    for which in ("u", "temp"):
        u = _randn_field(ins, sp, 66).requires_grad_(True)
        temp = _scalar_randn(ins, sp, 67).requires_grad_(True)
        F, Ftemp = _StageRightHandSide.apply(u, temp, 0.0, sp)
        with torch.no_grad():
            (u if which == "u" else temp).add_(1.0)
        with pytest.raises(RuntimeError):
            (F.sum() + Ftemp.sum()).backward()
    # and the whole step is differentiable in both fields
    u = _u0(ins, sp, ps, 68).requires_grad_(True)
    temp = _scalar_randn(ins, sp, 69).requires_grad_(True)
    gu, gt = torch.autograd.grad(step(u, temp), (u, temp))
    assert float(gu.abs().max()) > 0 and float(gt.abs().max()) > 0


# ------------------------------------------------------------------------------------ 8. the example
def test_rayleigh_benard_gradient_example(ins):
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("RayleighBenardGradient2D", os.path.join(ex, "RayleighBenardGradient2D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.main(n=16, nstep=10, dt=5e-3, verbose=False)
    print(f"Nu = {r['Nu']:.6f}, dJ = {r['dJ']:.9e}, fd = {r['fd']:.9e}")
    assert np.isfinite(r["Nu"]) and r["Nu"] > 0 and r["ghost"] == 0.0
    assert abs(r["fd"] - r["dJ"]) <= 1e-6 * abs(r["dJ"]), (r["fd"], r["dJ"])
