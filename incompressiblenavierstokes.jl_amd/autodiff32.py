"""Reverse-mode differentiability of the isothermal step with `T = Float32`, exported as `ins_amd.ad32`: `ins_amd.ad` over float32 fields, on the
`_f32` forwards (ins_amd.f32) and their pullbacks (csrc/ins_adjoint32.hip), each the exact transpose of its forward on the whole padded array
(DESIGN.md "Differentiability").

    st = ins.create_stepper(method, setup=setup, psolver=ins.f32.default_psolver32(setup), u=u0)        # u0: float32, requires_grad
    u = ad32.timestep(method, st, Δt).u
    (u * u).sum().backward()                                                                              # u0.grad = ∂loss/∂u0

A closure model given as a torch function `m(u, θ)` on float32 fields is added as F + m(u, θ); its parameters get gradients from torch.  What the `_f32`
family does not run raises NotImplementedError: a temperature field, the library's fused Smagorinsky closure, callable boundary data, an unsteady
body force, slab setups, and `psolver_wrap32` around `psolver_spectral` on an all-periodic box.
"""
import torch

from . import f32 as F32
from .boundary_conditions import HaloBC, PeriodicBC
from .setup import _fortran_strides
from .time_steppers import LMWray3, _lmwray3_as_erk, create_stepper

__all__ = ["apply_bc_u", "momentum", "project", "timestep"]


def _check_setup(setup, what):
    if any(isinstance(bc, HaloBC) for side in setup.boundary_conditions for bc in side):
        raise NotImplementedError(f"ad32.{what}: slab (halo) setups run in fp64 only")
    if setup.needs_bc_planes:
        raise NotImplementedError(f"ad32.{what}: the _f32 family takes constant boundary data (callable DirichletBC values: use ins_amd.ad)")
    if setup.bodyforce is not None and not setup.issteadybodyforce:
        raise NotImplementedError(f"ad32.{what}: an unsteady body force is evaluated in fp64 on the host (use ins_amd.ad)")
    m = setup.closure_model
    if m is not None and getattr(m, "_ins_closure", None) == "smagorinsky":
        raise NotImplementedError(f"ad32.{what}: the fused Smagorinsky closure is fp64 and has no pullback; give the closure as a torch function m(u, θ)")


def _check_psolver(setup, psolver, what):
    from .pressure import psolver_spectral

    if not isinstance(psolver, F32.psolver_spectral32):
        raise TypeError(f"ad32.{what} takes a Float32 pressure solver (f32.psolver_spectral32, f32.psolver_wrap32, f32.default_psolver32)")
    inner = getattr(psolver, "psolver64", None)
    if isinstance(inner, psolver_spectral) and all(isinstance(bc, PeriodicBC) for side in setup.boundary_conditions for bc in side):
        raise NotImplementedError(f"ad32.{what}: psolver_wrap32 around psolver_spectral on an all-periodic box is not taken; use f32.psolver_spectral32")


def _field(setup, x, vector):
    """`x` itself when it already is a float32 field in the library's layout, else a copy in that layout."""
    g = setup.grid
    shape = tuple(g.N) + ((g.dimension,) if vector else ())
    if x.dtype != torch.float32:
        raise TypeError("ad32 takes float32 torch tensors")
    if x.device == setup.device and tuple(x.shape) == shape and tuple(x.stride()) == _fortran_strides(shape):
        return x
    return _copy(setup, x, vector)


def _copy(setup, x, vector):
    """A fresh float32 field (library layout) holding `x`: the in-place forwards and pullbacks work on it."""
    if x.dtype != torch.float32:
        raise TypeError("ad32 takes float32 torch tensors")
    f = F32.vectorfield32(setup) if vector else F32.scalarfield32(setup)
    f.copy_(x.detach())
    return f


class _ApplyBCU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        return F32.apply_bc_u32_(_copy(setup, u, True), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.apply_bc_u_pullback32_(_copy(s, g, True), s), None


class _Momentum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        uf = _field(setup, u, True)
        # the input itself goes through save_for_backward (an in-place change before backward() raises); a layout copy is private
        if uf is u:
            ctx.save_for_backward(u)
            ctx.ucopy = None
        else:
            ctx.save_for_backward()
            ctx.ucopy = uf
        return F32.momentum32_(F32.vectorfield32(setup), uf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        u = ctx.saved_tensors[0] if ctx.ucopy is None else ctx.ucopy
        return F32.momentum_pullback32_(F32.vectorfield32(s), _field(s, g, True), u, s), None


class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, psolver):
        ctx.setup, ctx.psolver = setup, psolver
        return F32.project32_(_copy(setup, u, True), setup, psolver, F32.scalarfield32(setup))

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.project_pullback32_(_copy(s, g, True), s, ctx.psolver, F32.scalarfield32(s)), None, None


def apply_bc_u(u, t, setup):
    """boundary_conditions.jl:114-167 with T = Float32 and constant boundary data (`t` does not enter); pullback: apply_bc_u_pullback32_."""
    _check_setup(setup, "apply_bc_u")
    return _ApplyBCU.apply(u, setup)


def _bodyforce32(setup):
    f = getattr(setup, "_bodyforce32", None)
    if f is None or f[0] is not setup.bodyforce:
        f = (setup.bodyforce, F32.to_f32(setup, setup.bodyforce))
        setup._bodyforce32 = f
    return f[1]


def momentum(u, temp, t, setup):
    """operators.jl:940-976 with T = Float32, isothermal: convection + diffusion (momentum32_; the pullback is one launch) + a steady body
    force, which is additive and drops out of the pullback."""
    if temp is not None:
        raise NotImplementedError("ad32.momentum: the temperature equation has no Float32 pullbacks (use ins_amd.ad)")
    _check_setup(setup, "momentum")
    F = _Momentum.apply(u, setup)
    return F if setup.bodyforce is None else F + _bodyforce32(setup)


def project(u, setup, psolver):
    """pressure.jl:52-82 with T = Float32 (project32_); pullback: project_pullback32_, the transpose for this kind of solver."""
    _check_setup(setup, "project")
    _check_psolver(setup, psolver, "project")
    return _Project.apply(u, setup, psolver)


def timestep(method, stepper, Δt, θ=None):
    """step_explicit_runge_kutta.jl:61-120 with T = Float32: one explicit Runge-Kutta step without mutation, differentiable in `stepper.u`
    and (through a torch closure model `m(u, θ)`) in θ; `ad.timestep` on the Float32 operators, stage combinations in torch arithmetic."""
    setup, psolver, u, t, n = stepper.setup, stepper.psolver, stepper.u, stepper.t, stepper.n
    if stepper.temp is not None:
        raise NotImplementedError("ad32.timestep: the temperature equation has no Float32 pullbacks (use ins_amd.ad)")
    _check_setup(setup, "timestep")
    _check_psolver(setup, psolver, "timestep")
    m = setup.closure_model
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    A, c = erk.A, erk.c
    tstart, ustart, ku = t, u, []
    for i in range(len(erk.b)):
        u = apply_bc_u(u, t, setup)
        F = momentum(u, None, t, setup)
        if m is not None:
            F = F + m(u, θ)
        ku.append(F)
        t = tstart + c[i] * Δt
        u = ustart
        for j in range(i + 1):
            if A[i, j] != 0:
                u = u + (Δt * A[i, j]) * ku[j]
        u = apply_bc_u(u, t, setup)
        u = project(u, setup, psolver)
    u = apply_bc_u(u, t, setup)
    return create_stepper(method, setup=setup, psolver=psolver, u=u, t=t, n=n + 1)
