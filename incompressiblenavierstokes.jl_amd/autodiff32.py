"""Reverse-mode differentiability of the step with `T = Float32`, exported as `ins_amd.ad32`: `ins_amd.ad` over float32 fields, on the
`_f32` forwards (ins_amd.f32) and their pullbacks (csrc/ins_adjoint32.hip, csrc/ins_temp_adjoint32.hip), each the exact transpose of its forward on
the whole padded array (DESIGN.md "Differentiability").

    st = ins.create_stepper(method, setup=setup, psolver=ins.f32.default_psolver32(setup), u=u0)        # u0: float32, requires_grad
    u = ad32.timestep(method, st, Δt).u
    (u * u).sum().backward()                                                                              # u0.grad = ∂loss/∂u0

A closure model given as a torch function `m(u, θ)` on float32 fields is added as F + m(u, θ); its parameters get gradients from torch.  What the `_f32`
family does not run raises NotImplementedError: a temperature field on a setup without a temperature equation, the library's fused fp64 Smagorinsky
closure `ins_amd.smagorinsky_closure` (its differentiable Float32 form is `ad32.smagorinsky_closure`, below), callable boundary data (of the velocity
or of the temperature), an unsteady body force, slab setups, and `psolver_wrap32` around `psolver_spectral` on an all-periodic box.

With a temperature equation (`Setup(temperature=temperature_equation(...))`, constant boundary data) the step is differentiable in `stepper.temp`
too: `timestep` fills the ghosts of `temp` before each stage, a stage's right-hand side (u, temp) -> (F, Ftemp) is one Function whose backward is
two launches (`momentum_pullback32_`, then `temperature_pullback32_`), the `ktemp` combinations are torch arithmetic, and `momentum(u, temp, t,
setup)` adds the gravity term.  The operators are module attributes with the semantics of their `ad` namesakes on float32 tensors (they are not
in `__all__`):

    apply_bc_temp(temp, t, setup)                                 ghost fill of the temperature (`t` does not enter)
    gravity(temp, setup)                                          the vector field α2 avg(temp) e_gdir
    convection_diffusion_temp(u, temp, setup)                     differentiable in `u` and in `temp`
    dissipation(u, setup)                                         the pullback recomputes diffusion(u) in the kernel

The tensor-basis closure runs in Float32 too (csrc/ins_tensorclosure32.hip), through module attributes with the semantics of their `ad` namesakes on
float32 tensors (they are not in `__all__`):

    apply_bc_p(p, t, setup), apply_bc_p_fields(σ, t, setup)      ghost fill of a scalar field / of every channel of an N + (n,) field
    tensorinvariants(u, setup)                                    V, N + (nv,), written on Ip
    tensorclosure_stress(u, a, setup)                             τ = Σ_i a_i B_i(u), a symmetric tensorfield32; backward gives ubar and abar
    divoftensor(σ, setup), lastdimcontract(a, b)
    smagorinsky_closure(setup)                                    m(u, θ) with a learnable constant: a_2 = 2 θ² d² sqrt(2 V_1)

`neuralclosure.tensorclosure(..., dtype=torch.float32)` is built from them, and both are closure models for `ad32.timestep`.  A float64 tensor raises
TypeError, a field of another shape ValueError, a slab setup NotImplementedError.
"""
import numpy as np
import torch

from . import f32 as F32
from .boundary_conditions import HaloBC, PeriodicBC
from .setup import _fortran_strides
from .time_steppers import LMWray3, _lmwray3_as_erk, create_stepper

__all__ = ["apply_bc_u", "momentum", "project", "timestep"]


def _check_slab(setup, what):
    if any(isinstance(bc, HaloBC) for side in setup.boundary_conditions for bc in side):
        raise NotImplementedError(f"ad32.{what}: slab (halo) setups run in fp64 only")


def _check_setup(setup, what):
    _check_slab(setup, what)
    if setup.needs_bc_planes:
        raise NotImplementedError(f"ad32.{what}: the _f32 family takes constant boundary data (callable DirichletBC values: use ins_amd.ad)")
    if setup.bodyforce is not None and not setup.issteadybodyforce:
        raise NotImplementedError(f"ad32.{what}: an unsteady body force is evaluated in fp64 on the host (use ins_amd.ad)")
    m = setup.closure_model
    if m is not None and getattr(m, "_ins_closure", None) == "smagorinsky":
        raise NotImplementedError(f"ad32.{what}: the fused Smagorinsky closure is fp64 and has no pullback; use ad32.smagorinsky_closure(setup), "
                                  "or give the closure as a torch function m(u, θ)")


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
    """operators.jl:940-976 with T = Float32: convection + diffusion (momentum32_; the pullback is one launch) + a steady body force, which
    is additive and drops out of the pullback.  With a temperature field (and a temperature equation in `setup`) the gravity term is added
    (operators.jl:974), differentiable in `u` and in `temp`."""
    if temp is not None and setup.temperature is None:
        raise NotImplementedError("ad32.momentum: a temperature field needs setup.temperature (temperature_equation)")
    _check_setup(setup, "momentum")
    F = _Momentum.apply(u, setup)
    if temp is not None:
        F = F + gravity(temp, setup)
    return F if setup.bodyforce is None else F + _bodyforce32(setup)


# ------------------------------------------------------------------------------------ temperature equation
def _save_inputs(ctx, setup, items):
    """The fields a backward reads, `items` = (tensor, vector) pairs: an input that already is a library field goes through
    save_for_backward, so an in-place change of it before backward() raises; a layout copy is private to the Function."""
    fields, saved, copies = [], [], []
    for x, vector in items:
        f = _field(setup, x, vector)
        fields.append(f)
        if f is x:
            saved.append(x)
            copies.append(None)
        else:
            copies.append(f)
    ctx.save_for_backward(*saved)
    ctx.copies = copies
    return fields


def _saved_inputs(ctx):
    saved = list(ctx.saved_tensors)
    return [saved.pop(0) if c is None else c for c in ctx.copies]


class _ApplyBCTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, setup):
        ctx.setup = setup
        return F32.apply_bc_temp32_(_copy(setup, temp, False), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.apply_bc_temp_pullback32_(_copy(s, g, False), s), None


class _Gravity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, setup):
        ctx.setup = setup
        return F32.gravity32_(F32.vectorfield32(setup), _field(setup, temp, False), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.gravity_adjoint32_(F32.scalarfield32(s), _field(s, g, True), s), None


class _ConvectionDiffusionTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, temp, setup):
        ctx.setup = setup
        uf, tf = _save_inputs(ctx, setup, [(u, True), (temp, False)])
        return F32.convection_diffusion_temp32_(F32.scalarfield32(setup), uf, tf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        u, temp = _saved_inputs(ctx)
        ubar = F32.vectorfield32(s) if ctx.needs_input_grad[0] else None
        tempbar = F32.scalarfield32(s) if ctx.needs_input_grad[1] else None
        if ubar is not None or tempbar is not None:
            F32.convection_diffusion_temp_adjoint32_(ubar, tempbar, _field(s, g, False), u, temp, s)
        return ubar, tempbar, None


class _Dissipation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        (uf,) = _save_inputs(ctx, setup, [(u, True)])
        return F32.dissipation32_(F32.scalarfield32(setup), F32.vectorfield32(setup), uf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        (u,) = _saved_inputs(ctx)
        return F32.dissipation_adjoint32_(F32.vectorfield32(s), _field(s, g, False), u, s), None


class _StageRightHandSide(torch.autograd.Function):
    """(u, temp) -> (F, Ftemp) of one Runge-Kutta stage (step_explicit_runge_kutta.jl:79-83) with T = Float32: F = momentum(u, temp) without
    the body force, Ftemp = convection_diffusion_temp(u, temp) + dissipation(u).  The backward is two launches: momentum_pullback32_, then
    temperature_pullback32_."""

    @staticmethod
    def forward(ctx, u, temp, setup):
        ctx.setup = setup
        ctx.set_materialize_grads(False)
        uf, tf = _save_inputs(ctx, setup, [(u, True), (temp, False)])
        F = F32.momentum32_(F32.vectorfield32(setup), uf, setup, temp=tf)
        Ftemp = F32.convection_diffusion_temp32_(F32.scalarfield32(setup), uf, tf, setup)
        if setup.temperature.dodissipation:
            F32.dissipation32_(Ftemp, F32.vectorfield32(setup), uf, setup)
        return F, Ftemp

    @staticmethod
    def backward(ctx, gF, gT):
        s = ctx.setup
        if gF is None and gT is None:
            return None, None, None
        u, temp = _saved_inputs(ctx)
        Fbar = F32.vectorfield32(s) if gF is None else _field(s, gF, True)
        cbar = F32.scalarfield32(s) if gT is None else _field(s, gT, False)
        ubar = F32.momentum_pullback32_(F32.vectorfield32(s), Fbar, u, s)
        ubar, tempbar = F32.temperature_pullback32_(ubar, F32.scalarfield32(s), Fbar, cbar, u, temp, s)
        return ubar, tempbar, None


def _check_temperature(setup, what):
    _check_slab(setup, what)
    if setup.temperature is None:
        raise ValueError(f"ad32.{what} needs setup.temperature (temperature_equation)")


def apply_bc_temp(temp, t, setup):
    """boundary_conditions.jl:236-246 with T = Float32 and constant boundary data (`t` does not enter); pullback: apply_bc_temp_pullback32_."""
    _check_temperature(setup, "apply_bc_temp")
    return _ApplyBCTemp.apply(temp, setup)


def gravity(temp, setup):
    """operators.jl:884-931 with T = Float32; pullback: gravity_adjoint32_."""
    _check_temperature(setup, "gravity")
    return _Gravity.apply(temp, setup)


def convection_diffusion_temp(u, temp, setup):
    """operators.jl:692-737 with T = Float32, differentiable in `u` and in `temp`; pullback: convection_diffusion_temp_adjoint32_."""
    _check_temperature(setup, "convection_diffusion_temp")
    return _ConvectionDiffusionTemp.apply(u, temp, setup)


def dissipation(u, setup):
    """operators.jl:770-814 with T = Float32; the pullback (dissipation_adjoint32_) recomputes diffusion(u) in the kernel."""
    _check_temperature(setup, "dissipation")
    return _Dissipation.apply(u, setup)


def project(u, setup, psolver):
    """pressure.jl:52-82 with T = Float32 (project32_); pullback: project_pullback32_, the transpose for this kind of solver."""
    _check_setup(setup, "project")
    _check_psolver(setup, psolver, "project")
    return _Project.apply(u, setup, psolver)


# ------------------------------------------------------------------------------------ DNS-to-LES filters
class _Filter(torch.autograd.Function):
    """`v = Φ(u, setup_les, comp)` (lib/NeuralClosure filter.jl) on float32 fields with the exact transpose as backward (csrc/ins_filter32.hip):
    the Float32 twin of `ad.FaceAverage` / `ad.VolumeAverage`.  `Filter.apply(u, setup_les, comp, setup_dns=None)`."""

    _kind = None

    @classmethod
    def _filter(cls):
        from . import neuralclosure as nc

        return nc.FaceAverage() if cls._kind == "face" else nc.VolumeAverage()

    @classmethod
    def forward(cls, ctx, u, setup_les, comp, setup_dns=None):
        from .neuralclosure import dns_setup_of

        dns = setup_dns or dns_setup_of(setup_les, int(comp))
        ctx.les, ctx.dns, ctx.comp = setup_les, dns, int(comp)
        return cls._filter()(_field(dns, u.detach(), True), setup_les, int(comp), setup_dns=dns)

    @classmethod
    def backward(cls, ctx, g):
        ubar = cls._filter().pullback_(F32.vectorfield32(ctx.dns), _field(ctx.les, g, True), ctx.les, ctx.comp, ctx.dns)
        return ubar, None, None, None


class FaceAverage(_Filter):
    """filter.jl:26-46"""

    _kind = "face"


class VolumeAverage(_Filter):
    """filter.jl:82-116"""

    _kind = "volume"


# ------------------------------------------------------------------------------------ tensor-basis closure
def _vec(setup, u):
    """`u` as a float32 vector field in the library's layout; another dtype raises TypeError, another shape ValueError."""
    shape = tuple(setup.grid.N) + (setup.grid.dimension,)
    if u.dtype != torch.float32:
        raise TypeError("ad32 takes float32 torch tensors")
    if tuple(u.shape) != shape:
        raise ValueError(f"expected a field of shape {shape}, got {tuple(u.shape)}")
    return _field(setup, u, True)


def _nfield(setup, x, ncomp):
    """`x` as an N + (ncomp,) float32 field in the library's layout (a copy when it has another one)."""
    shape = tuple(setup.grid.N) + (ncomp,)
    if x.dtype != torch.float32:
        raise TypeError("ad32 takes float32 torch tensors")
    if tuple(x.shape) != shape:
        raise ValueError(f"expected a field of shape {shape}, got {tuple(x.shape)}")
    if x.device == setup.device and tuple(x.stride()) == _fortran_strides(shape):
        return x.detach()
    f = F32.nfield32(setup, ncomp)
    f.copy_(x.detach())
    return f


def _saved_field(ctx, setup, u):
    """The velocity a stencil reads, kept for backward: the input itself goes through save_for_backward (an in-place change before
    backward() raises); a layout copy is private to the Function."""
    uf = _vec(setup, u)
    if uf is u:
        ctx.save_for_backward(u)
        ctx.ucopy = None
    else:
        ctx.save_for_backward()
        ctx.ucopy = uf
    return uf


class _ApplyBCP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, setup):
        ctx.setup = setup
        return F32.apply_bc_p32_(_copy(setup, p, False), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.apply_bc_p_pullback32_(_copy(s, g, False), s), None


class _DivOfTensor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, σ, setup):
        ctx.setup = setup
        return F32.divoftensor32_(F32.vectorfield32(setup), _nfield(setup, σ, F32._tb_sizes(setup)[2]), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return F32.divoftensor_adjoint32_(F32.tensorfield32(s), _field(s, g, True), s), None


class _TensorInvariants(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        return F32.tensorinvariants32_(F32.nfield32(setup, F32._tb_sizes(setup)[1]), _saved_field(ctx, setup, u), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        u = ctx.saved_tensors[0] if ctx.ucopy is None else ctx.ucopy
        Vbar = _nfield(s, g, F32._tb_sizes(s)[1])
        return F32.tensorclosure_pullback32_(F32.vectorfield32(s), None, None, Vbar, u, None, s), None


class _TensorClosureStress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, a, setup):
        ctx.setup = setup
        uf = _vec(setup, u)
        af = _nfield(setup, a, F32._tb_sizes(setup)[0])
        # both inputs go through save_for_backward when they already are library fields: an in-place change before backward() raises
        ctx.ucopy = None if uf is u else uf
        ctx.acopy = None if af.data_ptr() == a.data_ptr() else af
        ctx.save_for_backward(*([u] if ctx.ucopy is None else []), *([a] if ctx.acopy is None else []))
        return F32.tensorclosure_stress32_(F32.tensorfield32(setup), uf, af, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        saved = list(ctx.saved_tensors)
        u = saved.pop(0) if ctx.ucopy is None else ctx.ucopy
        a = saved.pop(0).detach() if ctx.acopy is None else ctx.acopy
        nb, _, ns = F32._tb_sizes(s)
        abar = F32.nfield32(s, nb)
        ubar = F32.tensorclosure_pullback32_(F32.vectorfield32(s), abar, _nfield(s, g, ns), None, u, a, s)
        return ubar, abar, None


def apply_bc_p(p, t, setup):
    """boundary_conditions.jl:114-206 with T = Float32 (`t` does not enter); pullback: apply_bc_p_pullback32_."""
    _check_slab(setup, "apply_bc_p")
    if tuple(p.shape) != tuple(setup.grid.N):
        raise ValueError(f"expected a field of shape {tuple(setup.grid.N)}, got {tuple(p.shape)}")
    return _ApplyBCP.apply(p, setup)


def apply_bc_p_fields(σ, t, setup):
    """`apply_bc_p` on every channel of an N + (n,) field (the stress tensor's ghost fill, operators.jl:1296)."""
    if σ.dim() != setup.grid.dimension + 1:
        raise ValueError(f"expected a field of shape {tuple(setup.grid.N)} + (n,), got {tuple(σ.shape)}")
    return torch.stack([apply_bc_p(σ[..., q], t, setup) for q in range(σ.shape[-1])], dim=-1)


def tensorinvariants(u, setup):
    """The invariants V of the tensor basis (N + (nv,), written on Ip) with T = Float32, without forming B."""
    _check_slab(setup, "tensorinvariants")
    return _TensorInvariants.apply(u, setup)


def tensorclosure_stress(u, a, setup):
    """τ = Σ_i a_i B_i(u) as a symmetric `tensorfield32` (written on Ip) in one kernel that keeps the basis in registers; the backward gives
    ubar and abar_i = <τbar, B_i>.  `a` is N + (nb,)."""
    _check_slab(setup, "tensorclosure_stress")
    return _TensorClosureStress.apply(u, a, setup)


def divoftensor(σ, setup):
    """operators.jl:1155-1184 with T = Float32 (pullback: divoftensor_adjoint32_) on a symmetric `tensorfield32` N + (D(D+1)/2,)."""
    _check_slab(setup, "divoftensor")
    return _DivOfTensor.apply(σ, setup)


def lastdimcontract(a, b):
    """tensorbasis.jl:97-157: c[I] = Σ_i a[I, i] b[I, i, ...] — plain torch (its pullback is torch's)."""
    return (a.reshape(a.shape + (1,) * (b.dim() - a.dim())) * b).sum(dim=a.dim() - 1)


def smagorinsky_closure(setup):
    """Differentiable Smagorinsky closure `m(u, θ)` with T = Float32 (operators.jl:1284-1300), θ a 0-dim tensor: the member
    a_2 = 2 θ² d² sqrt(2 V_1), every other a_i = 0, of the tensor-basis family, as `ad.smagorinsky_closure`; gridsize² d² is held in float32."""
    _check_slab(setup, "smagorinsky_closure")
    g = setup.grid
    D = g.dimension
    nb = F32._tb_sizes(setup)[0]
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    pads = [q for α in reversed(range(D)) for q in (g.Ip[α][0], g.N[α] - g.Ip[α][1])]
    d2 = torch.zeros(tuple(g.N), dtype=torch.float64, device=setup.device)
    for α in range(D):
        shape = [1] * D
        shape[α] = g.N[α]
        d2 = d2 + torch.as_tensor(np.asarray(g.Δ[α], dtype=np.float64) ** 2, device=setup.device).reshape(shape)
    d2 = d2[ip].float()

    def closure(u, θ):
        θ = torch.as_tensor(θ, dtype=torch.float32, device=setup.device)
        V = tensorinvariants(u, setup)
        a2 = torch.nn.functional.pad(2 * θ * θ * d2 * torch.sqrt(2 * V[ip + (0,)]), pads)  # Ip only: sqrt has no derivative at the zeros outside
        z = torch.zeros_like(a2)
        a = torch.stack([z, a2] + [z] * (nb - 2), dim=-1)
        τ = apply_bc_p_fields(tensorclosure_stress(u, a, setup), 0.0, setup)
        return divoftensor(τ, setup)

    return closure


def timestep(method, stepper, Δt, θ=None):
    """step_explicit_runge_kutta.jl:61-120 with T = Float32: one explicit Runge-Kutta step without mutation, differentiable in `stepper.u`,
    in `stepper.temp` (with the temperature equation) and (through a torch closure model `m(u, θ)`) in θ; `ad.timestep` on the Float32
    operators, stage combinations in torch arithmetic.  With a temperature field the right-hand side of a stage, (u, temp) -> (F, Ftemp), is
    one Function whose backward is two launches."""
    setup, psolver, u, temp, t, n = stepper.setup, stepper.psolver, stepper.u, stepper.temp, stepper.t, stepper.n
    if temp is not None and setup.temperature is None:
        raise NotImplementedError("ad32.timestep: a temperature field needs setup.temperature (temperature_equation)")
    _check_setup(setup, "timestep")
    _check_psolver(setup, psolver, "timestep")
    m = setup.closure_model
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    A, c = erk.A, erk.c
    tstart, ustart, tempstart, ku, ktemp = t, u, temp, [], []
    for i in range(len(erk.b)):
        u = apply_bc_u(u, t, setup)
        if temp is None:
            F = momentum(u, None, t, setup)
        else:
            temp = apply_bc_temp(temp, t, setup)
            F, Ftemp = _StageRightHandSide.apply(u, temp, setup)
            if setup.bodyforce is not None:
                F = F + _bodyforce32(setup)
            ktemp.append(Ftemp)
        if m is not None:
            F = F + m(u, θ)
        ku.append(F)
        t = tstart + c[i] * Δt
        u = ustart
        for j in range(i + 1):
            if A[i, j] != 0:
                u = u + (Δt * A[i, j]) * ku[j]
        if temp is not None:
            temp = tempstart
            for j in range(i + 1):
                if A[i, j] != 0:
                    temp = temp + (Δt * A[i, j]) * ktemp[j]
        u = apply_bc_u(u, t, setup)
        u = project(u, setup, psolver)
    u = apply_bc_u(u, t, setup)
    if temp is not None:
        temp = apply_bc_temp(temp, t, setup)
    return create_stepper(method, setup=setup, psolver=psolver, u=u, temp=temp, t=t, n=n + 1)
