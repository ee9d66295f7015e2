"""GPU: the differentiable tensor-basis closure (csrc/ins_tensorclosure.hip, `ins_amd.ad`, `ins_amd.neuralclosure.tensorclosure`).

  1. the fused forward equals the composition of what exists (`ins.tensorbasis` + a contraction);
  2. `ad.smagorinsky_closure` equals `ins.smagorinsky_closure`;
  3. the pullbacks against the reference VJP of tests/tensorbasis_ref.py (oracle transposes by unit probes + torch.autograd of the pointwise map);
  4. the operator route and the fused route give the same ubar, abar_i = <full(taubar), B_i>;
  5. torch.autograd.gradcheck;  6. bitwise reproducibility and `accumulate`;  7. end to end through `ad.timestep` and a short training run;
  8. unsupported inputs raise.

`full(taubar)` is the D×D cotangent of the D(D+1)/2 stored entries of a symmetric tensor: off-diagonal entries halved on both sides
(tests/tensorbasis_ref.py).
"""
import numpy as np
import pytest

from tests import fixtures as fx
from tests import tensorbasis_ref as tr
from tests.test_gpu_adjoint import GEOMS, ORACLE_GEOMS, TOL, mirror, rand

pytestmark = pytest.mark.gpu

POLY_CAP = 1e-10  # the polynomial pullbacks: 10 x the observed error, capped here (a larger error is a bug)
POLY_BOUND = 5e-15  # 10 x the largest error observed (test_pullbacks_match_reference_vjp)


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def nfield(ins, sp, ncomp, seed):
    return ins.from_numpy(sp, fx.randn_field(tuple(sp.grid.N) + (ncomp,), seed))


def relmax_t(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def sizes(sp):
    return tr.sizes(sp.grid.dimension)


def full_cot(ins, sp, t):
    """N + (ns,) cotangent -> N + (D, D) torch tensor (off-diagonals halved)."""
    import torch

    return torch.as_tensor(tr.full_cotangent(ins.to_numpy(t)), device=sp.device)


# ------------------------------------------------------------------------------------ 1. fused forward = composition
@pytest.mark.parametrize("name", list(GEOMS))
def test_fused_forward_matches_tensorbasis(ins, oracle, name):
    import torch

    sp = mirror(ins, GEOMS[name](oracle), oracle)
    D = sp.grid.dimension
    nb, nv, ns = sizes(sp)
    u = rand(ins, sp, True, 100)
    a = nfield(ins, sp, nb, 101)
    B, V = ins.tensorbasis(u, sp)
    Vf = ins.tensorinvariants_(ins.from_numpy(sp, np.zeros(tuple(sp.grid.N) + (nv,))), u, sp)
    assert relmax_t(Vf, V) <= TOL
    tau = ins.tensorclosure_stress_(ins.tensorfield(sp), u, a, sp)
    Bm = ins.tensorbasis_matrices(B, sp)  # N + (nb, D, D)
    full = (a[..., None, None] * Bm).sum(dim=-3)
    ref = torch.stack([full[..., p, q] for p, q in tr.sym_pairs(D)], dim=-1)
    err = relmax_t(tau, ref)
    print(name, "stress vs composition:", err)
    assert err <= TOL
    # ad.lastdimcontract is that contraction
    assert relmax_t(ins.ad.lastdimcontract(a, Bm), full) <= TOL


# ------------------------------------------------------------------------------------ 2. Smagorinsky identity
@pytest.mark.parametrize("name", ["periodic32_3d", "periodic32_2d", "mixed", "box_symmetric", "box_pressure"])
def test_smagorinsky_identity(ins, oracle, name):
    import torch

    sp = mirror(ins, GEOMS[name](oracle), oracle)
    u = ins.apply_bc_u(rand(ins, sp, True, 110), 0.0, sp)
    θ = 0.17
    ref = ins.copyfield(ins.smagorinsky_closure(sp)(u, θ))
    got = ins.ad.smagorinsky_closure(sp)(u, torch.tensor(θ, dtype=torch.float64, device=sp.device))
    err = relmax_t(got, ref)
    print(name, "smagorinsky:", err)
    assert err <= TOL


# ------------------------------------------------------------------------------------ 3. pullbacks against the reference VJP
@pytest.mark.parametrize("name", ORACLE_GEOMS + ["setup3d"])
def test_pullbacks_match_reference_vjp(ins, oracle, name):
    """Observed on an MI355X (this test prints every figure): the relative max-norm errors of the polynomial pullbacks lie between 1.4e-16 and
    5.0e-16 on the six geometries (largest: tensorclosure_pullback, stress + invariants, on `mixed`: 4.96e-16; abar on the 7 x 7 boxes:
    4.94e-16; tensorbasis_pullback on setup3d: 4.65e-16), so POLY_BOUND is 10 x that, 5e-15, far under the 1e-10 cap.  The linear
    divoftensor_adjoint_ (observed <= 1.6e-16) is held to 1e-12."""
    o = oracle
    so = GEOMS[name](o)
    sp = mirror(ins, so, o)
    N, D = tuple(so.grid.N), so.grid.D
    nb, nv, ns = tr.sizes(D)
    u = fx.randn_field(N + (D,), 120)
    Bbar = fx.randn_field(N + (nb, D, D), 121)
    Vbar = fx.randn_field(N + (nv,), 122)
    a = fx.randn_field(N + (nb,), 123)
    taubar = fx.randn_field(N + (ns,), 124)
    sbar = fx.randn_field(N + (D,), 125)
    ug, Vg, ag, tg = (ins.from_numpy(sp, x) for x in (u, Vbar, a, taubar))
    Bg = ins.from_numpy(sp, tr.lib_B_from_oracle(Bbar))
    bound = min(POLY_BOUND, POLY_CAP)
    errs = {}

    # operator-level pullback: B part, V part, both
    for what, bb, vv in (("B", Bbar, None), ("V", None, Vbar), ("BV", Bbar, Vbar)):
        ref = tr.tensorbasis_vjp(o, so, u, bb, vv)
        got = ins.tensorbasis_pullback_(ins.vectorfield(sp), Bg if bb is not None else None, Vg if vv is not None else None, ug, sp)
        errs["tensorbasis_pullback " + what] = tr.relmax(ins.to_numpy(got), ref)
    # fused pullback: stress part, invariant part, both
    for what, has_a, vv in (("stress", True, None), ("invariants", False, Vbar), ("both", True, Vbar)):
        uref, aref = tr.closure_vjp(o, so, u, a if has_a else None, taubar if has_a else None, vv)
        abar = nfield(ins, sp, nb, 126) if has_a else None  # overwritten: the previous content must not matter
        got = ins.tensorclosure_pullback_(ins.vectorfield(sp), abar, tg if has_a else None, Vg if vv is not None else None, ug, ag if has_a else None, sp)
        errs["tensorclosure_pullback " + what] = tr.relmax(ins.to_numpy(got), uref)
        if has_a:
            errs["tensorclosure_pullback abar " + what] = tr.relmax(ins.to_numpy(abar), aref)
    for k, e in errs.items():
        print(f"{name}: {k}: {e:.3e}")
    # linear: divoftensor_adjoint_ (accumulates into zeros)
    ref = tr.divoftensor_transpose(o, so, sbar)
    got = ins.divoftensor_adjoint_(ins.tensorfield(sp), ins.from_numpy(sp, sbar), sp)
    elin = tr.relmax(ins.to_numpy(got), ref)
    print(f"{name}: divoftensor_adjoint: {elin:.3e}")
    assert elin <= TOL, elin
    assert max(errs.values()) <= bound, errs


@pytest.mark.parametrize("name", list(GEOMS))
def test_divoftensor_transpose_identity(ins, oracle, name):
    """<div σ, w> = <σ, divᵀ w> on the symmetric fields, on every geometry (PressureBC sides put DOFs into the ghost layer)."""
    check_divoftensor_transpose(ins, mirror(ins, GEOMS[name](oracle), oracle))


def check_divoftensor_transpose(ins, sp):
    ns = sizes(sp)[2]
    σ, w = nfield(ins, sp, ns, 130), rand(ins, sp, True, 131)
    s = ins.divoftensor_(ins.vectorfield(sp), σ, sp)
    σbar = ins.divoftensor_adjoint_(ins.tensorfield(sp), w, sp)
    lhs, rhs = float((s * w).sum()), float((σ * σbar).sum())
    assert abs(lhs - rhs) <= TOL * float(s.norm()) * float(w.norm()), (lhs, rhs)


# ------------------------------------------------------------------------------------ 4. the two routes agree
@pytest.mark.parametrize("name", ["setup3d", "mixed", "periodic32_3d"])
def test_operator_and_fused_routes_agree_3d(ins, oracle, name):
    import torch

    sp = mirror(ins, GEOMS[name](oracle), oracle)
    D = sp.grid.dimension
    nb, nv, ns = sizes(sp)
    u, a, taubar = rand(ins, sp, True, 140), nfield(ins, sp, nb, 141), nfield(ins, sp, ns, 142)
    abar = nfield(ins, sp, nb, 143)
    ub = ins.tensorclosure_pullback_(ins.vectorfield(sp), abar, taubar, None, u, a, sp)
    T = full_cot(ins, sp, taubar)  # N + (D, D)
    Bbar_m = a[..., None, None] * T[..., None, :, :]  # N + (nb, D, D), [..., i, p, q]
    Bbar = ins.from_numpy(sp, tr.lib_B_from_oracle(ins.to_numpy(Bbar_m)))
    ref = ins.tensorbasis_pullback_(ins.vectorfield(sp), Bbar, None, u, sp)
    assert relmax_t(ub, ref) <= TOL
    B, _ = ins.tensorbasis(u, sp)
    aref = (T[..., None, :, :] * ins.tensorbasis_matrices(B, sp)).sum(dim=(-1, -2))
    assert relmax_t(abar, aref) <= TOL
    assert torch.isfinite(ub).all()


# ------------------------------------------------------------------------------------ 5. gradcheck
def _small_setups(ins, oracle):
    x = (np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9))
    out = []
    for kind in ("PeriodicBC", "DirichletBC"):
        bc = getattr(oracle, kind)()
        out.append(mirror(ins, oracle.make_setup(x, ((bc, bc), (bc, bc)), Re=100.0), oracle))
    out.append(mirror(ins, fx.setup_periodic(oracle, 6, D=3), oracle))
    return out


def test_gradcheck(ins, oracle):
    import torch

    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-6)
    for sp in _small_setups(ins, oracle):
        nb, nv, ns = sizes(sp)
        # velocity scaled to ∇u = O(1) (h >= 1/8): with unit random velocities the degree-5 tensors are 1e5 times the degree-1 ones, and the
        # rounding of the finite differences of the former (1e-16 |τ| / eps) exceeds atol + rtol |J| of the latter
        u = (rand(ins, sp, True, 150) * 0.1).requires_grad_(True)
        a = nfield(ins, sp, nb, 151).requires_grad_(True)
        σ = nfield(ins, sp, ns, 152).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda uu, aa: ins.ad.tensorclosure_stress(uu, aa, sp), (u, a), **kw)
        assert torch.autograd.gradcheck(lambda uu: ins.ad.tensorbasis(uu, sp), (u,), **kw)
        assert torch.autograd.gradcheck(lambda uu: ins.ad.tensorinvariants(uu, sp), (u,), **kw)
        assert torch.autograd.gradcheck(lambda ss: ins.ad.divoftensor(ss, sp), (σ,), **kw)


# ------------------------------------------------------------------------------------ 6. reproducibility, accumulate
def test_reproducible_and_accumulate(ins, oracle):
    import torch

    sp = mirror(ins, GEOMS["periodic32_3d"](oracle), oracle)
    D = sp.grid.dimension
    nb, nv, ns = sizes(sp)
    u, a = rand(ins, sp, True, 160), nfield(ins, sp, nb, 161)
    taubar, Vbar, Bbar = nfield(ins, sp, ns, 162), nfield(ins, sp, nv, 163), nfield(ins, sp, nb * D * D, 164)
    sbar, base = rand(ins, sp, True, 165), rand(ins, sp, True, 166)

    def fused(out, acc=False):
        ab = nfield(ins, sp, nb, 167)
        return ins.tensorclosure_pullback_(out, ab, taubar, Vbar, u, a, sp, accumulate=acc), ab

    def oper(out, acc=False):
        return ins.tensorbasis_pullback_(out, Bbar, Vbar, u, sp, accumulate=acc), None

    for f in (fused, oper):
        (r1, a1), (r2, a2) = f(ins.vectorfield(sp)), f(ins.vectorfield(sp))
        assert torch.equal(r1, r2)
        if a1 is not None:
            assert torch.equal(a1, a2)
        acc, _ = f(ins.copyfield(base), acc=True)
        assert float((acc - (base + r1)).abs().max()) <= 1e-14 * float((base + r1).abs().max())
    d1 = ins.divoftensor_adjoint_(ins.tensorfield(sp), sbar, sp)
    d2 = ins.divoftensor_adjoint_(ins.tensorfield(sp), sbar, sp)
    assert torch.equal(d1, d2)
    tb = nfield(ins, sp, ns, 168)
    dacc = ins.divoftensor_adjoint_(ins.copyfield(tb), sbar, sp)
    assert float((dacc - (tb + d1)).abs().max()) <= 1e-14 * float((tb + d1).abs().max())


# ------------------------------------------------------------------------------------ 7. end to end
def _u0(ins, sp, ps, seed):
    u = ins.apply_bc_u(rand(ins, sp, True, seed), 0.0, sp)
    return ins.apply_bc_u(ins.project_(u, sp, ps, ins.scalarfield(sp)), 0.0, sp)


def _one_step_loss(ins, sp, ps, u0, θ):
    method = ins.RKMethods.RK44()
    u = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), 1e-3, θ=θ).u
    return (u * u).sum()


def test_timestep_gradient_wrt_mlp_parameters(ins, oracle):
    import torch

    sp = mirror(ins, GEOMS["periodic32_2d"](oracle), oracle)
    m = ins.neuralclosure.tensorclosure(setup=sp, hidden=[8, 8], activation=torch.tanh, rng=0)
    sp.closure_model = m
    ps = ins.default_psolver(sp)
    u0 = _u0(ins, sp, ps, 170)
    _one_step_loss(ins, sp, ps, u0, None).backward()
    for n, q in m.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all() and float(q.grad.abs().max()) > 0, n
    # a dict of parameters goes through functional_call and gets the same gradient
    θ = {n: q.detach().clone().requires_grad_(True) for n, q in m.named_parameters()}
    g = torch.autograd.grad(_one_step_loss(ins, sp, ps, u0, θ), list(θ.values()))
    for (n, q), gi in zip(m.named_parameters(), g):
        assert relmax_t(gi, q.grad) <= TOL, n


def test_timestep_gradient_wrt_smagorinsky_constant(ins, oracle):
    import torch

    sp = mirror(ins, GEOMS["periodic32_2d"](oracle), oracle)
    sp.closure_model = ins.ad.smagorinsky_closure(sp)
    ps = ins.default_psolver(sp)
    u0 = _u0(ins, sp, ps, 171)
    θ = torch.tensor(0.3, dtype=torch.float64, device=sp.device, requires_grad=True)
    (g,) = torch.autograd.grad(_one_step_loss(ins, sp, ps, u0, θ), θ)
    e = 1e-6
    with torch.no_grad():
        fd = float(_one_step_loss(ins, sp, ps, u0, θ + e) - _one_step_loss(ins, sp, ps, u0, θ - e)) / (2 * e)
    print("d loss / d θ:", float(g), "central difference:", fd)
    assert abs(float(g) - fd) <= 1e-6 + 1e-6 * abs(fd), (float(g), fd)


def test_wall_bounded_3d_step(ins, oracle):
    """The model is not periodic-only: one differentiable RK44 step on the 3-D Periodic x Dirichlet/Pressure x Symmetric box."""
    import torch

    sp = mirror(ins, GEOMS["mixed"](oracle), oracle)
    m = ins.neuralclosure.tensorclosure(setup=sp, hidden=[6], activation=torch.tanh, rng=1)
    with torch.no_grad():  # a small closure on a gentle field: the degree-5 tensors of a unit random field on this grid (h down to 0.05) overflow in a step
        m.layers[-1].weight.mul_(1e-3)
    sp.closure_model = m
    ps = ins.default_psolver(sp)
    u0 = (_u0(ins, sp, ps, 172) * 0.1).requires_grad_(True)
    loss = _one_step_loss(ins, sp, ps, u0, None)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(u0.grad).all() and float(u0.grad.abs().max()) > 0
    for n, q in m.named_parameters():
        assert q.grad is not None and torch.isfinite(q.grad).all() and float(q.grad.abs().max()) > 0, n
    # the native mutating step runs the same model without gradients
    method = ins.RKMethods.RK44()
    with torch.no_grad():
        ref = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0.detach()), 1e-3).u
        got = ins.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0.detach()), 1e-3).u
    assert relmax_t(got, ref) <= 1e-11


def test_short_posteriori_training(ins):
    """2-D, LES 32² from DNS 128², Adam, 20 iterations of the a-posteriori loss: the loss goes down."""
    import torch

    nc = ins.neuralclosure
    params = dict(D=2, Re=2000.0, lims=(0.0, 1.0), nles=[32], ndns=128, filters=(nc.FaceAverage(),), tburn=0.02, tsim=0.05, savefreq=5, Δt=5e-4)
    data = [nc.create_les_data(**params, rng=np.random.default_rng(s))[0] for s in (11, 12)]
    x = tuple(np.linspace(0.0, 1.0, 33) for _ in range(2))
    sp = ins.Setup(x=x, Re=2000.0)
    ps = ins.default_psolver(sp)
    method = ins.RKMethods.RK44()
    m = nc.tensorclosure(setup=sp, hidden=[8], activation=torch.tanh, rng=2)
    with torch.no_grad():  # start from a small closure (coefficients of the size of an eddy viscosity), as one would after scaling the invariants
        m.layers[-1].weight.mul_(1e-3)
    loss = nc.create_loss_post(setup=sp, method=method, psolver=ps, closure_model=m, nsubstep=5)
    loader = nc.create_dataloader_post([dict(u=d["u"], t=d["t"]) for d in data], ntrajectory=2, nunroll=3, device=sp.device)
    fixed, _ = loader(np.random.default_rng(0))
    with torch.no_grad():
        first = float(loss(fixed, None))
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    nc.train(dataloader=lambda rng: (fixed, rng), loss=loss, trainstate=dict(opt=opt, θ=None, rng=np.random.default_rng(1)), niter=20)
    with torch.no_grad():
        last = float(loss(fixed, None))
    relerr = nc.create_relerr_post(data=dict(u=data[0]["u"][..., :4], t=data[0]["t"][:4]), setup=sp, method=method, psolver=ps, closure_model=m, nsubstep=5)
    print("a-posteriori loss: first", first, "last", last, "relerr", relerr(None))
    assert last < first


# ------------------------------------------------------------------------------------ 8. unsupported inputs
def test_unsupported_inputs_raise(ins):
    import torch

    x = tuple(np.linspace(0.0, 1.0, 17) for _ in range(3))
    sp = ins.Setup(x=x, Re=1000.0)
    nb, nv, ns = sizes(sp)
    u = rand(ins, sp, True, 180)
    a = nfield(ins, sp, nb, 181)
    with pytest.raises(TypeError):
        ins.ad.tensorclosure_stress(u.float(), a.float(), sp)
    with pytest.raises(TypeError):
        ins.ad.tensorinvariants(u.float(), sp)
    with pytest.raises(TypeError):
        ins.ad.tensorbasis(u.float(), sp)
    with pytest.raises(TypeError):
        ins.tensorclosure_stress_(ins.tensorfield(sp), u.float(), a, sp)
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    slab = ins.Setup(x=x, Re=1000.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    us, as_ = rand(ins, slab, True, 182), nfield(ins, slab, nb, 183)
    with pytest.raises(ins.INSHipError):
        ins.ad.tensorclosure_stress(us, as_, slab)
    with pytest.raises(ins.INSHipError):
        ins.tensorbasis_pullback_(ins.vectorfield(slab), None, nfield(ins, slab, nv, 184), us, slab)
    with pytest.raises(ins.INSHipError):
        ins.divoftensor_adjoint_(ins.tensorfield(slab), us, slab)
    # no cotangent at all, and a without taubar
    with pytest.raises(ins.INSHipError):
        ins.tensorbasis_pullback_(ins.vectorfield(sp), None, None, u, sp)
    with pytest.raises(ins.INSHipError):
        ins.tensorclosure_pullback_(ins.vectorfield(sp), None, None, None, u, a, sp)
    # the saved velocity is version-checked
    uu = u.clone().requires_grad_(True)
    out = ins.ad.tensorclosure_stress(uu, a, sp)
    with torch.no_grad():
        uu.add_(1.0)
    with pytest.raises(RuntimeError):
        out.backward(torch.ones_like(out))
