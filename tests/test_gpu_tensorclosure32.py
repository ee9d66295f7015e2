"""GPU: the Float32 tensor-basis closure (csrc/ins_tensorclosure32.hip, `ins_amd.f32`, `ins_amd.ad32`, `neuralclosure.tensorclosure(dtype=float32)`).

  1. forwards (V, τ, divoftensor) against the fp64 twins on the same inputs promoted to double, per output field, max-norm relative to max|result|;
  2. pullbacks value by value against ins_tensorclosure_pullback_f64 / ins_divoftensor_adjoint_f64 on promoted inputs;
  3. transpose identities of the linear maps;  4. bitwise reproducibility;  5. ad32.smagorinsky_closure;  6. steps through ad32.timestep;
  7. refusals.

Yardsticks.  For V and τ: the CPU float32 evaluation of tests/tensorbasis_ref.pointwise on oracle.gradu(u) rounded to float32, against the
float64 evaluation on the unrounded gradient (for τ with the same coefficients `a`): what plain float32 arithmetic, input rounding included,
costs on these formulas at these gradients.  The kernel also forms ∇u in float from float-rounded reciprocals and orders the products
differently: margin MARGIN = 4 (tests/test_gpu_adjoint32.py).  divoftensor32_ has no pointwise twin: its yardstick is the error of momentum32_
against momentum_ on the same geometry, the same margin.  A pullback is held to MARGIN x the measured forward error of the same float kernel
family on the same geometry (the reverse sweep runs about twice the products): τ's for the stress cotangent and abar, V's for the invariants'
cotangent, the larger of the two for both together and for `accumulate`, divoftensor32_'s for its adjoint.  A transpose identity is held to the
forward yardstick itself, no margin (the smallest τ field's for the maps on the stress channels).

Fields, coefficients and cotangents are random multiples of 2^-10 over the whole padded array.  Every test prints `RATIO ...` (measured
error / yardstick) before it asserts.  The forward results of a geometry are computed once and shared by tests 1, 2, 3 and 5."""
import numpy as np
import pytest

from tests import fixtures as fx
from tests import tensorbasis_ref as tr
from tests.test_gpu_adjoint32 import (DT, GEOMS, MARGIN, STEP_CASES, _ke, _solvers_for_step, _steps, _u0, defect, dot, mirror, nrm, pair,
                                      rell2, relmax, yard_momentum)

pytestmark = pytest.mark.gpu

THETA = 0.171875  # 11/64: the same Smagorinsky constant in float32 and float64
USCALE = 0.125    # start fields of the step tests: a unit random field has |∇u|^5 ~ 1e6 on the mixed box, which a step does not survive


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def npair(ins, sp, ncomp, seed):
    """The same random N + (ncomp,) field, multiples of 2^-10, in float32 and in float64."""
    a = np.round(fx.randn_field(tuple(sp.grid.N) + (ncomp,), seed) * 1024.0) / 1024.0
    return ins.f32.to_f32(sp, a), ins.from_numpy(sp, a)


def zeros64(ins, sp, ncomp):
    return ins.from_numpy(sp, np.zeros(tuple(sp.grid.N) + (ncomp,)))


def cpu_relmax(a, b):
    return float((a.double() - b).abs().max()) / float(b.abs().max())


def per_field(got, ref):
    return [relmax(got[..., q], ref[..., q]) for q in range(ref.shape[-1])]


class Forward:
    """Inputs, fp64 and Float32 forward results, yardsticks and measured forward errors of one geometry."""


_FORWARD = {}


def forward(ins, oracle, name):
    if name in _FORWARD:
        return _FORWARD[name]
    import torch

    F = ins.f32
    d = Forward()
    d.so = GEOMS[name](oracle)
    d.sp = sp = mirror(ins, d.so, oracle)
    D = sp.grid.dimension
    d.nb, d.nv, d.ns = nb, nv, ns = tr.sizes(D)
    d.ip = ip = tuple(slice(lo, hi) for lo, hi in d.so.grid.Ip)
    d.u32, d.u64 = pair(ins, sp, True, 201)
    d.a32, d.a64 = npair(ins, sp, nb, 202)
    d.s32, d.s64 = npair(ins, sp, ns, 203)
    # the fp64 twins and the float kernels
    d.V64 = ins.tensorinvariants_(zeros64(ins, sp, nv), d.u64, sp)
    d.tau64 = ins.tensorclosure_stress_(ins.tensorfield(sp), d.u64, d.a64, sp)
    d.div64 = ins.divoftensor_(ins.vectorfield(sp), d.s64, sp)
    d.V32 = F.tensorinvariants32_(F.nfield32(sp, nv), d.u32, sp)
    d.tau32 = F.tensorclosure_stress32_(F.tensorfield32(sp), d.u32, d.a32, sp)
    d.div32 = F.divoftensor32_(F.vectorfield32(sp), d.s32, sp)
    # CPU yardstick: the pointwise formulas in float32 on the rounded gradient against float64 on the gradient itself
    d.G64 = torch.from_numpy(np.ascontiguousarray(oracle.gradu(ins.to_numpy(d.u64), d.so)))
    d.G32 = d.G64.float()
    d.B64, Vs64 = tr.pointwise(d.G64)
    d.B32, Vs32 = tr.pointwise(d.G32)
    d.Vs64, d.Vs32 = Vs64, Vs32
    at64 = torch.from_numpy(np.ascontiguousarray(ins.to_numpy(d.a64)[ip]))
    at32 = at64.float()
    t64 = sum(at64[..., i, None, None] * b for i, b in enumerate(d.B64))
    t32 = sum(at32[..., i, None, None] * b for i, b in enumerate(d.B32))
    assert t32.dtype == torch.float32 and Vs32[0].dtype == torch.float32
    d.yard_V = [cpu_relmax(Vs32[q], Vs64[q]) for q in range(nv)]
    d.yard_tau = [cpu_relmax(t32[..., p, r], t64[..., p, r]) for p, r in tr.sym_pairs(D)]
    d.Em = yard_momentum(ins, sp)
    # measured forward errors of the float kernels
    d.err_V = per_field(d.V32, d.V64)
    d.err_tau = per_field(d.tau32, d.tau64)
    d.err_div = per_field(d.div32, d.div64)
    _FORWARD[name] = d
    return d


def report(name, what, err, yard):
    """A uniform power-of-two box with fields on the 2^-10 lattice is exact in both precisions: error 0 against yardstick 0 is ratio 0."""
    ratio = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"RATIO {name} {what} err={err:.3e} yardstick={yard:.3e} ratio={ratio:.3f}")


def check(name, rows, margin):
    for what, err, yard in rows:
        report(name, what, err, yard)
    for what, err, yard in rows:
        assert err <= margin * yard, (what, err, yard)


# ------------------------------------------------------------------------------------ 1. forwards against the fp64 twins
@pytest.mark.parametrize("name", list(GEOMS))
def test_forwards_against_fp64(ins, oracle, name):
    d = forward(ins, oracle, name)
    rows = [(f"forward V[{q}]", d.err_V[q], d.yard_V[q]) for q in range(d.nv)]
    rows += [(f"forward tau[{q}]", d.err_tau[q], d.yard_tau[q]) for q in range(d.ns)]
    rows += [(f"forward divoftensor[{q}]", e, d.Em) for q, e in enumerate(d.err_div)]
    assert float(d.V64.abs().max()) > 0 and float(d.tau64.abs().max()) > 0 and float(d.div64.abs().max()) > 0
    # nothing is written outside Ip / Iu
    outside = d.V32.clone()
    outside[d.ip] = 0
    assert float(outside.abs().max()) == 0.0
    check(name, rows, MARGIN)


# ------------------------------------------------------------------------------------ 2. pullbacks against the fp64 twins
@pytest.mark.parametrize("name", list(GEOMS))
def test_pullbacks_against_fp64(ins, oracle, name):
    F = ins.f32
    d = forward(ins, oracle, name)
    sp, nb, nv, ns = d.sp, d.nb, d.nv, d.ns
    t32, t64 = npair(ins, sp, ns, 211)
    v32, v64 = npair(ins, sp, nv, 212)
    b32, b64 = pair(ins, sp, True, 213)
    w32, w64 = pair(ins, sp, True, 214)
    g32, g64 = npair(ins, sp, ns, 215)
    Et, Ev, Ed = max(d.err_tau), max(d.err_V), max(d.err_div)
    rows = []

    def both(has_a, has_v, acc=False):
        ab32, ab64 = npair(ins, sp, nb, 216) if has_a else (None, None)  # overwritten: the previous content must not matter
        out32 = b32.clone() if acc else F.vectorfield32(sp)
        out64 = b64.clone() if acc else ins.vectorfield(sp)
        F.tensorclosure_pullback32_(out32, ab32, t32 if has_a else None, v32 if has_v else None, d.u32, d.a32 if has_a else None, sp, accumulate=acc)
        ins.tensorclosure_pullback_(out64, ab64, t64 if has_a else None, v64 if has_v else None, d.u64, d.a64 if has_a else None, sp, accumulate=acc)
        return out32, out64, ab32, ab64

    o32, o64, ab32, ab64 = both(True, False)
    rows.append(("pullback ubar[taubar]", relmax(o32, o64), Et))
    rows += [(f"pullback abar[{q}]", e, Et) for q, e in enumerate(per_field(ab32, ab64))]
    o32, o64, _, _ = both(False, True)
    rows.append(("pullback ubar[Vbar]", relmax(o32, o64), Ev))
    o32, o64, ab32b, _ = both(True, True)
    rows.append(("pullback ubar[taubar+Vbar]", relmax(o32, o64), max(Et, Ev)))
    assert bool((ab32b == ab32).all())  # abar does not depend on Vbar
    o32, o64, _, _ = both(True, True, acc=True)
    rows.append(("pullback ubar[accumulate]", relmax(o32, o64), max(Et, Ev)))
    s32 = F.divoftensor_adjoint32_(g32.clone(), w32, sp)
    s64 = ins.divoftensor_adjoint_(g64.clone(), w64, sp)
    rows += [(f"pullback divoftensor_adjoint[{q}]", e, Ed) for q, e in enumerate(per_field(s32 - g32, s64 - g64))]
    check(name, rows, MARGIN)


# ------------------------------------------------------------------------------------ 3. transpose identities
@pytest.mark.parametrize("name", list(GEOMS))
def test_transpose_identities(ins, oracle, name):
    import torch

    F = ins.f32
    d = forward(ins, oracle, name)
    sp, nb, ns = d.sp, d.nb, d.ns
    w32, w64 = pair(ins, sp, True, 221)
    t32, t64 = npair(ins, sp, ns, 222)
    p32, p64 = npair(ins, sp, ns, 223)
    rows = []
    # divoftensor32_ and its adjoint
    LTw = F.divoftensor_adjoint32_(F.tensorfield32(sp), w32, sp)
    rows.append(("transpose divoftensor", defect(d.div32, d.s64, w64, LTw), d.Em))
    # a -> tau at fixed u, and abar
    abar = F.nfield32(sp, nb)
    F.tensorclosure_pullback32_(F.vectorfield32(sp), abar, t32, None, d.u32, d.a32, sp)
    rows.append(("transpose stress[a]", defect(d.tau32, d.a64, t64, abar), min(d.yard_tau)))
    # apply_bc_p per channel and its pullback
    x = p32.clone().requires_grad_(True)
    Lx = ins.ad32.apply_bc_p_fields(x, 0.0, sp)
    (LTt,) = torch.autograd.grad(Lx, x, t32)
    assert LTt.dtype == torch.float32 and nrm(Lx) > 0
    rows.append(("transpose apply_bc_p_fields", defect(Lx.detach(), p64, t64, LTt), min(d.yard_tau)))
    check(name, rows, 1.0)


# ------------------------------------------------------------------------------------ 4. bitwise reproducibility
@pytest.mark.parametrize("name", ["mixed", "box70"])
def test_pullbacks_reproducible(ins, oracle, name):
    import torch

    F = ins.f32
    d = forward(ins, oracle, name)
    sp, nb, nv, ns = d.sp, d.nb, d.nv, d.ns
    t32, _ = npair(ins, sp, ns, 231)
    v32, _ = npair(ins, sp, nv, 232)
    w32, _ = pair(ins, sp, True, 233)
    b32, _ = pair(ins, sp, True, 234)

    def run(has_a, has_v, acc):
        ab = F.nfield32(sp, nb) if has_a else None
        out = b32.clone() if acc else F.vectorfield32(sp)
        F.tensorclosure_pullback32_(out, ab, t32 if has_a else None, v32 if has_v else None, d.u32, d.a32 if has_a else None, sp, accumulate=acc)
        return out, ab

    for has_a, has_v, acc in ((True, False, False), (False, True, False), (True, True, False), (True, True, True)):
        (r1, a1), (r2, a2) = run(has_a, has_v, acc), run(has_a, has_v, acc)
        assert float(r1.abs().max()) > 0 and torch.equal(r1, r2), (has_a, has_v, acc)
        if has_a:
            assert float(a1.abs().max()) > 0 and torch.equal(a1, a2)
    s1 = F.divoftensor_adjoint32_(F.tensorfield32(sp), w32, sp)
    s2 = F.divoftensor_adjoint32_(F.tensorfield32(sp), w32, sp)
    assert float(s1.abs().max()) > 0 and torch.equal(s1, s2)
    print(f"RATIO {name} reproducible: every pullback bitwise equal on two calls")


# ------------------------------------------------------------------------------------ 5. ad32.smagorinsky_closure
@pytest.mark.parametrize("name", list(GEOMS))
def test_smagorinsky_closure(ins, oracle, name):
    """Value: the yardstick is the CPU float32 evaluation of τ = 2 θ² d² sqrt(2 V_1) S against float64 (largest field) plus the divoftensor
    yardstick (momentum32_ against momentum_), the two stages of the chain.  Gradients of ½‖c‖²: MARGIN x the measured error of the value."""
    import torch

    from ins_amd.autodiff import _gridsize2

    d = forward(ins, oracle, name)
    sp = d.sp
    D = sp.grid.dimension
    assert float(d.V64[d.ip + (0,)].min()) > 0  # V_1 > 0 on Ip: sqrt(2 V_1) is differentiated there
    d2 = _gridsize2(sp)[d.ip].cpu()
    a64 = 2 * THETA * THETA * d2 * torch.sqrt(2 * d.Vs64[0])
    a32 = (2 * np.float32(THETA) * np.float32(THETA)) * d2.float() * torch.sqrt(2 * d.Vs32[0])
    assert a32.dtype == torch.float32
    t64, t32 = a64[..., None, None] * d.B64[1], a32[..., None, None] * d.B32[1]
    yard = max(cpu_relmax(t32[..., p, r], t64[..., p, r]) for p, r in tr.sym_pairs(D)) + d.Em
    u32 = d.u32.clone().requires_grad_(True)
    u64 = d.u64.clone().requires_grad_(True)
    θ32 = torch.tensor(THETA, dtype=torch.float32, device=sp.device, requires_grad=True)
    θ64 = torch.tensor(THETA, dtype=torch.float64, device=sp.device, requires_grad=True)
    c32 = ins.ad32.smagorinsky_closure(sp)(u32, θ32)
    c64 = ins.ad.smagorinsky_closure(sp)(u64, θ64)
    assert c32.dtype == torch.float32
    errs = per_field(c32.detach(), c64.detach())
    gu32, gθ32 = torch.autograd.grad(_ke(c32), (u32, θ32))
    gu64, gθ64 = torch.autograd.grad(_ke(c64), (u64, θ64))
    assert gu32.dtype == torch.float32 and gθ32.dtype == torch.float32 and float(gu64.abs().max()) > 0 and float(gθ64) != 0
    Ec = max(errs)
    rows = [(f"smagorinsky value[{q}]", e, yard) for q, e in enumerate(errs)]
    rows.append(("smagorinsky gradient_u", relmax(gu32, gu64), Ec))
    rows.append(("smagorinsky gradient_theta", abs(float(gθ32) - float(gθ64)) / abs(float(gθ64)), Ec))
    check(name, rows, MARGIN)


# ------------------------------------------------------------------------------------ 6. steps through ad32.timestep
def _models(ins, sp32, sp64, model):
    """(θ32, θ64, parameters32, parameters64) with the closure models set on the two setups; the same float32-representable weights."""
    import torch

    if model == "smagorinsky":
        sp32.closure_model = ins.ad32.smagorinsky_closure(sp32)
        sp64.closure_model = ins.ad.smagorinsky_closure(sp64)
        θ32 = torch.tensor(THETA, dtype=torch.float32, device=sp32.device, requires_grad=True)
        θ64 = torch.tensor(THETA, dtype=torch.float64, device=sp64.device, requires_grad=True)
        return θ32, θ64, [θ32], [θ64]
    nc = ins.neuralclosure
    m64 = nc.tensorclosure(setup=sp64, hidden=[8], activation=torch.tanh, rng=3)
    m32 = nc.tensorclosure(setup=sp32, hidden=[8], activation=torch.tanh, rng=3, dtype=torch.float32)
    with torch.no_grad():
        m64.layers[-1].weight.mul_(1e-3)
        for a, b in zip(m64.parameters(), m32.parameters()):
            b.copy_(a)
            a.copy_(b)
    assert all(q.dtype == torch.float32 for q in m32.parameters())
    sp32.closure_model, sp64.closure_model = m32, m64
    return None, None, list(m32.parameters()), list(m64.parameters())


def _flat(gs):
    import torch

    return torch.cat([g.reshape(-1).double() for g in gs])


@pytest.mark.parametrize("model", ["smagorinsky", "tensorclosure"])
@pytest.mark.parametrize("name,kind", STEP_CASES)
def test_steps_gradients(ins, oracle, name, kind, model):
    import torch

    sp32 = mirror(ins, GEOMS[name](oracle), oracle)
    sp64 = mirror(ins, GEOMS[name](oracle), oracle)
    ps32 = _solvers_for_step(ins, sp32, kind)[0]
    ps64 = _solvers_for_step(ins, sp64, kind)[1]
    u32, u64 = _u0(ins, sp64, ps64, 240)
    u32, u64 = (u32 * USCALE).requires_grad_(True), (u64 * USCALE).requires_grad_(True)
    θ32, θ64, q32, q64 = _models(ins, sp32, sp64, model)
    out32 = _steps(ins, ins.ad32, sp32, ps32, u32, θ32)
    out64 = _steps(ins, ins.ad, sp64, ps64, u64, θ64)
    assert out32.dtype == torch.float32
    yard = rell2(out32.detach(), out64.detach())
    g32 = torch.autograd.grad(_ke(out32), [u32] + q32)
    g64 = torch.autograd.grad(_ke(out64), [u64] + q64)
    assert all(g.dtype == torch.float32 for g in g32)
    f32θ, f64θ = _flat(g32[1:]), _flat(g64[1:])
    assert bool(torch.isfinite(f32θ).all()) and float(f64θ.norm()) > 0 and float(g64[0].norm()) > 0
    # the closure acts: without it the final state differs by far more than the two precisions do
    sp64.closure_model = None
    with torch.no_grad():
        effect = rell2(_steps(ins, ins.ad, sp64, ps64, u64.detach()), out64.detach())
    print(f"RATIO {name} {model} steps: closure effect on u_N = {effect:.3e}, float32-vs-fp64 = {yard:.3e}")
    rows = [(f"steps[{model}] gradient_u0", rell2(g32[0], g64[0]), yard),
            (f"steps[{model}] gradient_theta", float((f32θ - f64θ).norm()) / float(f64θ.norm()), yard)]
    check(name, rows, MARGIN)
    assert effect > 0


def test_steps_taylor(ins, oracle):
    """First-order Taylor remainder of J(u0 + h v) through three Float32 steps with the Smagorinsky closure: a factor 4 per halving of h."""
    import torch

    name, kind = STEP_CASES[0]
    sp32 = mirror(ins, GEOMS[name](oracle), oracle)
    sp64 = mirror(ins, GEOMS[name](oracle), oracle)
    ps32 = _solvers_for_step(ins, sp32, kind)[0]
    ps64 = _solvers_for_step(ins, sp64, kind)[1]
    _models(ins, sp32, sp64, "smagorinsky")
    θ32 = torch.tensor(THETA, dtype=torch.float32, device=sp32.device)
    θ64 = torch.tensor(THETA, dtype=torch.float64, device=sp64.device)
    u32, u64 = _u0(ins, sp64, ps64, 241)
    v32, _ = _u0(ins, sp64, ps64, 242)
    u32, u64 = u32 * USCALE, u64 * USCALE
    v32 = v32 * (float(u32.norm()) / float(v32.norm()))
    uu = u32.clone().requires_grad_(True)
    J0t = _ke(_steps(ins, ins.ad32, sp32, ps32, uu, θ32))
    (g,) = torch.autograd.grad(J0t, uu)
    J0, dJ = float(J0t.detach()), dot(g, v32)
    with torch.no_grad():
        noise = abs(J0 - float(_ke(_steps(ins, ins.ad, sp64, ps64, u64, θ64))))  # the forward rounding of J
        hs = [0.2, 0.1, 0.05]
        r = [abs(float(_ke(_steps(ins, ins.ad32, sp32, ps32, u32 + h * v32, θ32))) - J0 - h * dJ) for h in hs]
    ratios = [r[k] / r[k + 1] for k in range(2)]
    print(f"RATIO {name} taylor[smagorinsky] J0={J0:.6e} dJ={dJ:.6e} noise={noise:.3e} remainders={r} ratios={ratios}")
    assert min(r) > 100 * noise, (r, noise)
    assert all(3.9 <= x <= 4.1 for x in ratios), (r, ratios)


def test_loss_post_float32(ins, oracle):
    """create_loss_post over ad32.timestep: with a Float32 pressure solver and a float32 model the a-posteriori loss is a float32 scalar,
    differentiable in the model's parameters, and agrees with the fp64 loss of the same weights.  The reference states are unrelated random
    fields, so the loss is O(1) and depends smoothly on the states: a relative state error ε moves it by at most about 4 ε, and three
    Float32 steps stay within 1e-5 of fp64 (tests/test_gpu_adjoint32.py prints 1e-7 .. 1e-6), hence 1e-4."""
    import torch

    name, kind = STEP_CASES[0]
    sp32 = mirror(ins, GEOMS[name](oracle), oracle)
    sp64 = mirror(ins, GEOMS[name](oracle), oracle)
    ps32 = _solvers_for_step(ins, sp32, kind)[0]
    ps64 = _solvers_for_step(ins, sp64, kind)[1]
    _, _, q32, _ = _models(ins, sp32, sp64, "tensorclosure")
    m32, m64 = sp32.closure_model, sp64.closure_model
    sp32.closure_model = sp64.closure_model = None
    states = torch.stack([_u0(ins, sp64, ps64, 250 + k)[1] * USCALE for k in range(3)], dim=-1)
    data = [dict(u=states, t=np.array([0.0, DT, 2 * DT]))]
    method = ins.RKMethods.RK44()
    nc = ins.neuralclosure
    l32 = nc.create_loss_post(setup=sp32, method=method, psolver=ps32, closure_model=m32)(data, None)
    l64 = nc.create_loss_post(setup=sp64, method=method, psolver=ps64, closure_model=m64)(data, None)
    g = torch.autograd.grad(l32, q32)
    rel = abs(float(l32) - float(l64)) / abs(float(l64))
    print(f"RATIO {name} loss_post float32={float(l32):.8e} fp64={float(l64):.8e} rel={rel:.3e}")
    assert l32.dtype == torch.float32 and all(x.dtype == torch.float32 and bool(torch.isfinite(x).all()) for x in g)
    assert float(_flat(g).norm()) > 0
    assert rel <= 1e-4


# ------------------------------------------------------------------------------------ 7. refusals
def test_refusals(ins):
    import torch

    F, A = ins.f32, ins.ad32
    x = tuple(np.linspace(0.0, 1.0, 9) for _ in range(3))
    sp = ins.Setup(x=x, Re=100.0)
    nb, nv, ns = tr.sizes(3)
    u, a, σ, p = F.vectorfield32(sp), F.nfield32(sp, nb), F.tensorfield32(sp), F.scalarfield32(sp)
    # float32 inputs run
    A.tensorinvariants(u, sp), A.tensorclosure_stress(u, a, sp), A.divoftensor(σ, sp), A.apply_bc_p(p, 0.0, sp), A.apply_bc_p_fields(σ, 0.0, sp)
    for call in (lambda: A.tensorinvariants(u.double(), sp), lambda: A.tensorclosure_stress(u.double(), a, sp),
                 lambda: A.tensorclosure_stress(u, a.double(), sp), lambda: A.divoftensor(σ.double(), sp), lambda: A.apply_bc_p(p.double(), 0.0, sp),
                 lambda: A.apply_bc_p_fields(σ.double(), 0.0, sp), lambda: A.smagorinsky_closure(sp)(u.double(), 0.1),
                 lambda: F.tensorinvariants32_(F.nfield32(sp, nv), u.double(), sp)):
        with pytest.raises(TypeError):
            call()
    for call in (lambda: A.tensorclosure_stress(u, F.nfield32(sp, nb - 1), sp), lambda: A.divoftensor(F.nfield32(sp, ns + 1), sp),
                 lambda: A.tensorinvariants(F.nfield32(sp, 2), sp), lambda: A.apply_bc_p(σ, 0.0, sp),
                 lambda: F.divoftensor32_(F.vectorfield32(sp), F.nfield32(sp, ns - 1), sp)):
        with pytest.raises(ValueError):
            call()
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    slab = ins.Setup(x=x, Re=100.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    us, as_, σs, ps_ = F.vectorfield32(slab), F.nfield32(slab, nb), F.tensorfield32(slab), F.scalarfield32(slab)
    for call in (lambda: A.tensorinvariants(us, slab), lambda: A.tensorclosure_stress(us, as_, slab), lambda: A.divoftensor(σs, slab),
                 lambda: A.apply_bc_p(ps_, 0.0, slab), lambda: A.apply_bc_p_fields(σs, 0.0, slab), lambda: A.smagorinsky_closure(slab)):
        with pytest.raises(NotImplementedError):
            call()
    # the C entry points refuse a slab grid with INS_ERR_UNSUPPORTED, an in-place pullback with INS_ERR_INVALID
    for call in (lambda: F.tensorinvariants32_(F.nfield32(slab, nv), us, slab), lambda: F.tensorclosure_stress32_(σs, us, as_, slab),
                 lambda: F.divoftensor32_(us, σs, slab), lambda: F.divoftensor_adjoint32_(σs, us, slab),
                 lambda: F.tensorclosure_pullback32_(F.vectorfield32(slab), None, None, F.nfield32(slab, nv), us, None, slab),
                 lambda: F.tensorclosure_pullback32_(u, None, None, F.nfield32(sp, nv), u, None, sp),
                 lambda: F.tensorclosure_pullback32_(F.vectorfield32(sp), None, None, None, u, a, sp)):
        with pytest.raises(ins.INSHipError):
            call()
    # the library's fused fp64 closure stays refused by ad32.timestep, and the message names the Float32 one
    sp.closure_model = ins.smagorinsky_closure(sp)
    method = ins.RKMethods.RK44()
    st = ins.create_stepper(method, setup=sp, psolver=F.psolver_spectral32(sp), u=u)
    with pytest.raises(NotImplementedError, match="ad32.smagorinsky_closure"):
        A.timestep(method, st, 1e-3)
    # the saved velocity is version-checked
    sp.closure_model = None
    uu = u.clone().requires_grad_(True)
    out = A.tensorclosure_stress(uu, a, sp)
    with torch.no_grad():
        uu.add_(1.0)
    with pytest.raises(RuntimeError):
        out.backward(torch.ones_like(out))
