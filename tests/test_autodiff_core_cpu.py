"""The shared autograd layer (`ins_amd._autodiff_core`) on the CPU, without the native library: a stub precision table of plain torch maps with
hand-written transposes, a stub setup, and the same step written directly in differentiable torch operations as the reference.

The stub maps: the ghost fills multiply by a fixed 0/1 mask; momentum is F = -u·u + ν (roll(u, 1, 0) - u); gravity averages `temp` along `gdir`;
the temperature terms are c = -u_0 temp + α4 (roll(temp, 1, 0) - temp) and γ Σ_α u_α²; project multiplies the first axis by a fixed symmetric matrix.

Tolerances (relative, 2-norm): 1e-12 in float64 (both sides do the same arithmetic, in another association order at most; a missing stage term is
an error of order 1) and 1e-5 in float32 (measured here: at most 1.7e-7 over all cases, so the bound set beforehand holds with room)."""
from types import SimpleNamespace

import pytest
import torch

ν, α2, α4, γ, GDIR = 0.05, 0.7, 0.03, 0.2, 1
SHAPES = {2: (6, 5), 3: (5, 4, 6)}
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}


@pytest.fixture(scope="module")
def core():
    import ins_amd

    return ins_amd._autodiff_core


def colmajor(shape, dtype):
    return torch.zeros(tuple(reversed(shape)), dtype=dtype).permute(*reversed(range(len(shape))))


def rand(shape, dtype, seed):
    """A random field in the library's (column-major) layout."""
    f = colmajor(shape, dtype)
    f.copy_(torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)))
    return f


# ------------------------------------------------------------------------------------ the maps, in differentiable torch
def mom(u):
    return -u * u + ν * (torch.roll(u, 1, 0) - u)


def grav(temp, D):
    e = torch.zeros(D, dtype=temp.dtype)
    e[GDIR] = 1
    return (α2 * 0.5 * (temp + torch.roll(temp, -1, GDIR))).unsqueeze(-1) * e


def cdt(u, temp):
    return -u[..., 0] * temp + α4 * (torch.roll(temp, 1, 0) - temp)


def diss(u):
    return γ * (u * u).sum(-1)


def proj(P, u):
    return torch.einsum("ij,j...->i...", P, u)


def make(D, dtype, temperature, bodyforce=False, closure=None):
    """(setup, ops): the stub setup and the stub precision table, `ops.calls` logging the pullbacks that ran."""
    N = SHAPES[D]
    grid = SimpleNamespace(N=N, dimension=D, Ip=tuple((1, n - 1) for n in N))
    gen = torch.Generator().manual_seed(7)
    setup = SimpleNamespace(grid=grid, device=torch.device("cpu"), temperature=SimpleNamespace(dodissipation=True) if temperature else None,
                            closure_model=closure, bodyforce=rand(N + (D,), dtype, 11) if bodyforce else None, boundary_conditions=(),
                            needs_bc_planes=False)
    setup.masku = (torch.rand(N + (D,), generator=gen) > 0.3).to(dtype)
    setup.maskp = (torch.rand(N, generator=gen) > 0.3).to(dtype)
    P = torch.randn(N[0], N[0], dtype=torch.float64, generator=gen)
    setup.P = ((P + P.T) / 4).to(dtype)
    calls = []

    def momentum_(F, u, temp, t, s):
        F.copy_(mom(u))
        return F if temp is None else F.add_(grav(temp, D))

    def gravity_adjoint_(tempbar, φ, s):
        return tempbar.add_(α2 * 0.5 * (φ[..., GDIR] + torch.roll(φ[..., GDIR], 1, GDIR)))

    def cdt_adjoint_(ubar, tempbar, cbar, u, temp, s):
        calls.append(("cdt_adjoint", ubar is None, tempbar is None))
        if ubar is not None:
            ubar[..., 0].add_(-temp * cbar)
        if tempbar is not None:
            tempbar.add_(-u[..., 0] * cbar + α4 * (torch.roll(cbar, -1, 0) - cbar))
        return ubar, tempbar

    def dissipation_adjoint_(ubar, cbar, u, s):
        return ubar.add_(2 * γ * u * cbar.unsqueeze(-1))

    def momentum_pullback_(ubar, φ, u, s):
        calls.append(("momentum_pullback",))
        return ubar.copy_(-2 * u * φ + ν * (torch.roll(φ, -1, 0) - φ))

    def temperature_pullback_(ubar, tempbar, Fbar, cbar, u, temp, s):
        calls.append(("temperature_pullback",))
        gravity_adjoint_(tempbar.zero_(), Fbar, s)
        tempbar.add_(-u[..., 0] * cbar + α4 * (torch.roll(cbar, -1, 0) - cbar))
        ubar[..., 0].add_(-temp * cbar)
        if s.temperature.dodissipation:
            dissipation_adjoint_(ubar, cbar, u, s)
        return ubar, tempbar

    def check_dtype(x):
        if x.dtype != dtype:
            raise TypeError("stub table: wrong dtype")

    ops = SimpleNamespace(
        name="stub", dtype=dtype, calls=calls, check_dtype=check_dtype, bodyforce=lambda s: s.bodyforce,
        scalarfield=lambda s: colmajor(N, dtype), vectorfield=lambda s: colmajor(N + (D,), dtype),
        apply_bc_u_=lambda u, t, s, dudt: u.mul_(s.masku), apply_bc_u_pullback_=lambda g, s: g.mul_(s.masku),
        apply_bc_temp_=lambda x, t, s: x.mul_(s.maskp), apply_bc_temp_pullback_=lambda g, s: g.mul_(s.maskp),
        momentum_=momentum_, momentum_pullback_=momentum_pullback_,
        gravity_=lambda F, temp, s: F.add_(grav(temp, D)), gravity_adjoint_=gravity_adjoint_,
        convection_diffusion_temp_=lambda c, u, temp, s: c.add_(cdt(u, temp)), convection_diffusion_temp_adjoint_=cdt_adjoint_,
        dissipation_=lambda d, diff, u, s: d.add_(diss(u)), dissipation_adjoint_=dissipation_adjoint_, temperature_pullback_=temperature_pullback_,
        project_=lambda u, s, ps, p: u.copy_(proj(s.P, u)), project_pullback_=lambda g, s, ps, p: g.copy_(proj(s.P, g)),
    )
    return setup, ops


def plain_step(erk, setup, u, temp, Δt, θ):
    """`core.timestep` in differentiable torch operations, no custom Function."""
    D, m = setup.grid.dimension, setup.closure_model
    ustart, tempstart, ku, ktemp = u, temp, [], []
    for i in range(len(erk.b)):
        u = u * setup.masku
        F = mom(u)
        if temp is not None:
            temp = temp * setup.maskp
            F = F + grav(temp, D)
            ktemp.append(cdt(u, temp) + diss(u))
        if setup.bodyforce is not None:
            F = F + setup.bodyforce
        if m is not None:
            F = F + m(u, θ)
        ku.append(F)
        u = ustart
        for j in range(i + 1):
            if erk.A[i, j] != 0:
                u = u + (Δt * erk.A[i, j]) * ku[j]
        if temp is not None:
            temp = tempstart
            for j in range(i + 1):
                if erk.A[i, j] != 0:
                    temp = temp + (Δt * erk.A[i, j]) * ktemp[j]
        u = proj(setup.P, u * setup.masku)
    return u * setup.masku, None if temp is None else temp * setup.maskp


def close(a, b, dtype):
    err = float((a.double() - b.double()).norm() / b.double().norm())
    print(f"relative error {err:.3e}")
    return err <= TOL[dtype]


def closure_model(u, θ):
    return θ[0] * torch.roll(u, 1, 1) * u + θ[1] * u


# ------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("with_closure", [False, True])
@pytest.mark.parametrize("with_temp", [False, True])
@pytest.mark.parametrize("method", ["RK44", "LMWray3"])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_timestep_matches_plain_torch(core, dtype, D, method, with_temp, with_closure):
    import ins_amd as ins

    setup, ops = make(D, dtype, with_temp, bodyforce=(D == 3), closure=closure_model if with_closure else None)
    meth = ins.RKMethods.RK44() if method == "RK44" else ins.LMWray3()
    erk = meth if method == "RK44" else ins.time_steppers._lmwray3_as_erk(meth)
    N = SHAPES[D]
    w, wt = rand(N + (D,), dtype, 3), rand(N, dtype, 4)
    out = []
    for step in ("core", "plain"):
        u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
        t0 = rand(N, dtype, 2).requires_grad_(True) if with_temp else None
        θ = torch.tensor([0.3, -0.2], dtype=dtype, requires_grad=True) if with_closure else None
        if step == "core":
            st = core.timestep(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=u0, temp=t0, t=0.25, n=3), 0.1, θ)
            assert st.n == 4 and st.t == pytest.approx(0.35)
            u, temp = st.u, st.temp
        else:
            u, temp = plain_step(erk, setup, u0, t0, 0.1, θ)
        loss = (u * u * w).sum() + (0 if temp is None else (temp * temp * wt).sum())
        loss.backward()
        out.append([x for x in (u.detach(), None if temp is None else temp.detach(), u0.grad, None if t0 is None else t0.grad,
                                None if θ is None else θ.grad) if x is not None])
    assert len(out[0]) == 2 + 2 * with_temp + with_closure
    for a, b in zip(*out):
        assert a.dtype == dtype and close(a, b, dtype)


# ------------------------------------------------------------------------------------ what is kept for backward
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_library_layout_input_is_saved_and_guarded(core, dtype):
    setup, ops = make(2, dtype, False)
    leaf = rand(SHAPES[2] + (2,), dtype, 1).requires_grad_(True)
    v = leaf.clone()  # keeps the column-major strides
    assert v.stride() == leaf.stride() and core._field(ops, setup, v, True) is v
    F = core._Momentum.apply(v, 0.0, setup, ops)
    with torch.no_grad():
        v.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        F.sum().backward()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_other_layout_input_is_copied(core, dtype):
    setup, ops = make(2, dtype, False)
    x = torch.randn(SHAPES[2] + (2,), dtype=dtype, generator=torch.Generator().manual_seed(1))  # torch's default strides
    w = rand(SHAPES[2] + (2,), dtype, 5)
    grads = []
    for change in (False, True):
        leaf = x.clone().requires_grad_(True)
        v = leaf.clone()
        assert core._field(ops, setup, v, True) is not v
        F = core._Momentum.apply(v, 0.0, setup, ops)
        if change:
            with torch.no_grad():
                v.add_(1.0)
        (F * w).sum().backward()
        grads.append(leaf.grad)
    assert torch.equal(grads[0], grads[1])
    ref = x.clone().requires_grad_(True)
    (mom(ref) * w).sum().backward()
    assert close(grads[0], ref.grad, dtype)


def test_wrong_dtype_goes_through_the_tables_hook(core):
    setup, ops = make(2, torch.float32, False)
    with pytest.raises(TypeError, match="stub table"):
        core._Momentum.apply(rand(SHAPES[2] + (2,), torch.float64, 1), 0.0, setup, ops)
    with pytest.raises(ValueError, match="expected a field of shape"):
        core._field(ops, setup, torch.zeros(SHAPES[2] + (4,), dtype=torch.float32), 3)


# ------------------------------------------------------------------------------------ cotangents that are absent, partial or expanded
@pytest.mark.parametrize("use", ["F", "Ftemp", "both"])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_stage_right_hand_side_with_partial_cotangents(core, dtype, D, use):
    setup, ops = make(D, dtype, True)
    N = SHAPES[D]
    w, wt = rand(N + (D,), dtype, 3), rand(N, dtype, 4)
    grads = []
    for step in ("core", "plain"):
        u, temp = rand(N + (D,), dtype, 1).requires_grad_(True), rand(N, dtype, 2).requires_grad_(True)
        if step == "core":
            F, Ftemp = core._StageRightHandSide.apply(u, temp, 0.0, setup, ops)
        else:
            F, Ftemp = mom(u) + grav(temp, D), cdt(u, temp) + diss(u)
        loss = ((F * w).sum() if use != "Ftemp" else 0) + ((Ftemp * wt).sum() if use != "F" else 0)
        loss.backward()
        grads.append((u.grad, temp.grad if temp.grad is not None else torch.zeros_like(temp)))
    assert ops.calls == [("momentum_pullback",), ("temperature_pullback",)]
    for a, b in zip(*grads):
        assert close(a, b, dtype) if float(b.norm()) > 0 else float(a.norm()) == 0


def test_stage_right_hand_side_without_cotangents_returns_none(core):
    setup, ops = make(2, torch.float64, True)
    u, temp = rand(SHAPES[2] + (2,), torch.float64, 1).requires_grad_(True), rand(SHAPES[2], torch.float64, 2).requires_grad_(True)
    F, _ = core._StageRightHandSide.apply(u, temp, 0.0, setup, ops)
    assert core._StageRightHandSide.backward(F.grad_fn, None, None) == (None,) * 5
    assert ops.calls == []


@pytest.mark.parametrize("which", [0, 1])
def test_convection_diffusion_temp_skips_the_half_nobody_needs(core, which):
    setup, ops = make(3, torch.float64, True)
    N = SHAPES[3]
    xs = [rand(N + (3,), torch.float64, 1), rand(N, torch.float64, 2)]
    xs[which].requires_grad_(True)
    w = rand(N, torch.float64, 3)
    (core._ConvectionDiffusionTemp.apply(xs[0], xs[1], setup, ops) * w).sum().backward()
    assert ops.calls == [("cdt_adjoint", which != 0, which != 1)]
    ref = [x.detach().clone().requires_grad_(x.requires_grad) for x in xs]
    (cdt(*ref) * w).sum().backward()
    assert xs[1 - which].grad is None and close(xs[which].grad, ref[which].grad, torch.float64)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_expanded_cotangent(core, dtype):
    """`.sum().backward()` hands the Function a cotangent with zero strides: it is copied into the library's layout."""
    setup, ops = make(3, dtype, True)
    N = SHAPES[3]
    u, temp = rand(N + (3,), dtype, 1).requires_grad_(True), rand(N, dtype, 2).requires_grad_(True)
    F, Ftemp = core._StageRightHandSide.apply(u, temp, 0.0, setup, ops)
    (core._ApplyBCU.apply(F, 0.0, setup, False, ops).sum() + Ftemp.sum()).backward()
    ur, tr = rand(N + (3,), dtype, 1).requires_grad_(True), rand(N, dtype, 2).requires_grad_(True)
    (((mom(ur) + grav(tr, 3)) * setup.masku).sum() + (cdt(ur, tr) + diss(ur)).sum()).backward()
    assert close(u.grad, ur.grad, dtype) and close(temp.grad, tr.grad, dtype)
