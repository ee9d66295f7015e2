"""Reverse-mode differentiability (the reference's ChainRules rrules, operators.jl:100-616, boundary_conditions.jl:114-230, pressure.jl:15-19,
sciml.jl:49-113) as `torch.autograd.Function`s, exported as `ins_amd.ad`.

Every function here has the signature of its allocating twin in `ins_amd` and the same forward result; its backward runs the pullback kernels of
csrc/ins_adjoint.hip and csrc/ins_temp_adjoint.hip (the temperature equation, which the reference's rules do not cover), each the exact transpose of the forward operator on the whole padded array (DESIGN.md "Differentiability").
`ad.timestep` is the non-mutating Runge-Kutta step of step_explicit_runge_kutta.jl:61-120 built from them, so

    u = ad.timestep(method, stepper, Δt).u
    loss = (u * u).sum(); loss.backward()          # stepper.u.grad = ∂loss/∂u0

`ad.timesteps(method, stepper, Δt, nsteps)` is `nsteps` of them as ONE Function for closure-free isothermal rollouts: the forward is the native
multi-step call in chunks, only the chunk-start states are kept, and the backward recomputes a chunk and runs one native call per reversed step
(csrc/ins_rk_adjoint.hip).

A closure model given as a torch function `m(u, θ)` is added as F + m(u, θ), and its parameters get gradients from torch.
"""
import numpy as np
import torch

from . import operators as O
from .boundary_conditions import DirichletBC
from .pressure import project_, project_pullback_
from .setup import _fortran_strides, scalarfield, vectorfield
from .time_steppers import LMWray3, _lmwray3_as_erk, create_stepper

__all__ = ["apply_bc_u", "apply_bc_p", "apply_bc_temp", "gravity", "convection_diffusion_temp", "dissipation", "scalewithvolume", "divergence", "pressuregradient", "applypressure", "poisson", "convection", "diffusion",
           "momentum", "project", "right_hand_side", "create_right_hand_side", "timestep", "timesteps", "FaceAverage", "VolumeAverage", "tensorbasis", "divoftensor",
           "lastdimcontract", "tensorinvariants", "tensorclosure_stress", "apply_bc_p_fields", "smagorinsky_closure"]


def _field(setup, x, vector):
    """`x` itself when it already has the library's field layout, else a copy in that layout (cotangents from torch are often expanded
    views with zero strides, or permuted the other way)."""
    g = setup.grid
    shape = tuple(g.N) + ((g.dimension,) if vector else ())
    if (x.dtype == torch.float64 and x.device == setup.device and tuple(x.shape) == shape and tuple(x.stride()) == _fortran_strides(shape)):
        return x
    return _copy(setup, x, vector)


def _saved_field(ctx, setup, u):
    """The velocity a stencil reads, kept for backward: the input itself goes through save_for_backward, so an in-place change of it
    before backward() raises instead of giving a wrong gradient; a layout copy is private to the Function."""
    uf = _field(setup, u, True)
    if uf is u:
        ctx.save_for_backward(u)
        ctx.ucopy = None
    else:
        ctx.save_for_backward()
        ctx.ucopy = uf
    return uf


def _saved(ctx):
    return ctx.saved_tensors[0] if ctx.ucopy is None else ctx.ucopy


def _copy(setup, x, vector):
    """A fresh field (library layout) holding `x`: the pullbacks work in place on it."""
    f = vectorfield(setup) if vector else scalarfield(setup)
    f.copy_(x.detach())
    return f


# ------------------------------------------------------------------------------------ ghost fill
class _ApplyBCU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, t, setup, dudt):
        ctx.setup = setup
        return O.apply_bc_u_(_copy(setup, u, True), t, setup, dudt=dudt)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.apply_bc_u_pullback_(_copy(s, g, True), 0.0, s), None, None, None


class _ApplyBCP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, setup):
        ctx.setup = setup
        return O.apply_bc_p_(_copy(setup, p, False), t, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.apply_bc_p_pullback_(_copy(s, g, False), 0.0, s), None, None


def apply_bc_u(u, t, setup, dudt=False):
    """boundary_conditions.jl:114-167 (rrule: apply_bc_u_pullback!)"""
    return _ApplyBCU.apply(u, t, setup, bool(dudt))


def apply_bc_p(p, t, setup):
    """boundary_conditions.jl:114-206 (rrule: apply_bc_p_pullback!)"""
    return _ApplyBCP.apply(p, t, setup)


# ------------------------------------------------------------------------------------ linear operators
class _ScaleWithVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, setup):
        ctx.setup = setup
        return O.scalewithvolume_(_copy(setup, p, False), setup)

    @staticmethod
    def backward(ctx, g):  # diagonal over the whole padded array
        s = ctx.setup
        return O.scalewithvolume_(_copy(s, g, False), s), None


class _Divergence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        return O.divergence(_field(setup, u, True), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.divergence_adjoint_(vectorfield(s), _field(s, g, False), s), None


class _PressureGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, setup):
        ctx.setup = setup
        return O.pressuregradient(_field(setup, p, False), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.pressuregradient_adjoint_(scalarfield(s), _field(s, g, True), s), None


class _ApplyPressure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, p, setup):
        ctx.setup = setup
        return O.applypressure_(_copy(setup, u, True), _field(setup, p, False), setup)

    @staticmethod
    def backward(ctx, g):  # u − G p: (φ, −Gᵀφ)
        s = ctx.setup
        gf = _field(s, g, True)
        pbar = O.pressuregradient_adjoint_(scalarfield(s), gf, s).neg_()
        return g, pbar, None


class _Poisson(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, psolver):
        ctx.psolver = psolver
        return psolver(_copy(psolver.setup, f, False))

    @staticmethod
    def backward(ctx, g):  # the solve is symmetric on the padded arrays (pressure.jl:15-19)
        ps = ctx.psolver
        return ps(_copy(ps.setup, g, False)), None


def scalewithvolume(p, setup):
    """operators.jl:81-95"""
    return _ScaleWithVolume.apply(p, setup)


def divergence(u, setup):
    """operators.jl:97-125 (rrule: divergence_adjoint!)"""
    return _Divergence.apply(u, setup)


def pressuregradient(p, setup):
    """operators.jl:149-178 (rrule: pressuregradient_adjoint!)"""
    return _PressureGradient.apply(p, setup)


def applypressure(u, p, setup):
    """operators.jl:203-233.  The pullbacks are φ for u and −Gᵀφ for p (not the reference's rrule, which drops the first and flips
    the sign of the second)."""
    return _ApplyPressure.apply(u, p, setup)


def poisson(psolver, f):
    """pressure.jl:15-19: the solve is its own pullback."""
    return _Poisson.apply(f, psolver)


# ------------------------------------------------------------------------------------ momentum
class _Convection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        uf = _saved_field(ctx, setup, u)
        return O.convection(uf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.convection_adjoint_(vectorfield(s), _field(s, g, True), _saved(ctx), s), None


class _Diffusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, use_viscosity):
        ctx.setup, ctx.use_viscosity = setup, use_viscosity
        return O.diffusion(_field(setup, u, True), setup, use_viscosity)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.diffusion_adjoint_(vectorfield(s), _field(s, g, True), s, ctx.use_viscosity), None, None


class _Momentum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, t, setup):
        ctx.setup = setup
        uf = _saved_field(ctx, setup, u)
        return O.momentum(uf, None, t, setup)

    @staticmethod
    def backward(ctx, g):  # the body force is additive: it drops out
        s = ctx.setup
        return O.momentum_pullback_(vectorfield(s), _field(s, g, True), _saved(ctx), s), None, None


def convection(u, setup):
    """operators.jl:366-415 (rrule: convection_adjoint!)"""
    return _Convection.apply(u, setup)


def diffusion(u, setup, use_viscosity=True):
    """operators.jl:521-573 (rrule: diffusion_adjoint!)"""
    return _Diffusion.apply(u, setup, bool(use_viscosity))


def momentum(u, temp, t, setup):
    """operators.jl:940-976 (convection + diffusion + body force; the pullback is one fused kernel).  With a temperature field the gravity term
    is added (operators.jl:974), differentiable in `u` and in `temp`."""
    if temp is None:
        return _Momentum.apply(u, t, setup)
    if setup.temperature is None:
        raise NotImplementedError("ad.momentum: a temperature field needs setup.temperature (temperature_equation)")
    return _Momentum.apply(u, t, setup) + gravity(temp, setup)


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
    def forward(ctx, temp, t, setup):
        ctx.setup = setup
        return O.apply_bc_temp_(_copy(setup, temp, False), t, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.apply_bc_temp_pullback_(_copy(s, g, False), 0.0, s), None, None


class _Gravity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, setup):
        ctx.setup = setup
        return O.gravity(_field(setup, temp, False), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.gravity_adjoint_(scalarfield(s), _field(s, g, True), s), None


class _ConvectionDiffusionTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, temp, setup):
        ctx.setup = setup
        uf, tf = _save_inputs(ctx, setup, [(u, True), (temp, False)])
        return O.convection_diffusion_temp(uf, tf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        u, temp = _saved_inputs(ctx)
        ubar = vectorfield(s) if ctx.needs_input_grad[0] else None
        tempbar = scalarfield(s) if ctx.needs_input_grad[1] else None
        if ubar is not None or tempbar is not None:
            O.convection_diffusion_temp_adjoint_(ubar, tempbar, _field(s, g, False), u, temp, s)
        return ubar, tempbar, None


class _Dissipation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        (uf,) = _save_inputs(ctx, setup, [(u, True)])
        return O.dissipation(uf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        (u,) = _saved_inputs(ctx)
        return O.dissipation_adjoint_(vectorfield(s), _field(s, g, False), u, s), None


class _StageRightHandSide(torch.autograd.Function):
    """(u, temp) -> (F, Ftemp) of one Runge-Kutta stage (step_explicit_runge_kutta.jl:79-83): F = momentum(u, temp), Ftemp =
    convection_diffusion_temp(u, temp) + dissipation(u).  The backward is two launches: momentum_pullback_, then temperature_pullback_."""

    @staticmethod
    def forward(ctx, u, temp, t, setup):
        ctx.setup = setup
        ctx.set_materialize_grads(False)
        uf, tf = _save_inputs(ctx, setup, [(u, True), (temp, False)])
        F = O.momentum_(vectorfield(setup), uf, tf, t, setup)
        Ftemp = O.convection_diffusion_temp_(scalarfield(setup), uf, tf, setup)
        if setup.temperature.dodissipation:
            O.dissipation_(Ftemp, vectorfield(setup), uf, setup)
        return F, Ftemp

    @staticmethod
    def backward(ctx, gF, gT):
        s = ctx.setup
        if gF is None and gT is None:
            return None, None, None, None
        u, temp = _saved_inputs(ctx)
        Fbar = vectorfield(s) if gF is None else _field(s, gF, True)
        cbar = scalarfield(s) if gT is None else _field(s, gT, False)
        ubar = O.momentum_pullback_(vectorfield(s), Fbar, u, s)
        ubar, tempbar = O.temperature_pullback_(ubar, scalarfield(s), Fbar, cbar, u, temp, s)
        return ubar, tempbar, None, None


def _need_temperature(setup, what):
    if setup.temperature is None:
        raise ValueError(f"ad.{what} needs setup.temperature (temperature_equation)")


def apply_bc_temp(temp, t, setup):
    """boundary_conditions.jl:236-246 (rrule: apply_bc_temp_pullback!)"""
    _need_temperature(setup, "apply_bc_temp")
    return _ApplyBCTemp.apply(temp, t, setup)


def gravity(temp, setup):
    """operators.jl:884-931 (rrule: gravity_adjoint!)"""
    _need_temperature(setup, "gravity")
    return _Gravity.apply(temp, setup)


def convection_diffusion_temp(u, temp, setup):
    """operators.jl:692-737, differentiable in `u` and in `temp` (the reference's rrule, :699-704, returns undefined names)."""
    _need_temperature(setup, "convection_diffusion_temp")
    return _ConvectionDiffusionTemp.apply(u, temp, setup)


def dissipation(u, setup):
    """operators.jl:770-814 (the reference's rrule is @test_broken); the pullback recomputes diffusion(u) in the kernel."""
    _need_temperature(setup, "dissipation")
    return _Dissipation.apply(u, setup)


# ------------------------------------------------------------------------------------ projection and right-hand side
class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, psolver):
        ctx.setup, ctx.psolver = setup, psolver
        return project_(_copy(setup, u, True), setup, psolver, scalarfield(setup))

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return project_pullback_(_copy(s, g, True), s, ctx.psolver, scalarfield(s)), None, None


class _RightHandSide(torch.autograd.Function):
    """project(bc_dudt(momentum(bc(u)))) forward and backward, each as one sequence of native calls on the setup's stream."""

    @staticmethod
    def forward(ctx, u, t, setup, psolver):
        ctx.setup, ctx.psolver = setup, psolver
        tmp = O.apply_bc_u_(_copy(setup, u, True), t, setup)
        dudt = O.momentum_(vectorfield(setup), tmp, None, t, setup)
        O.apply_bc_u_(dudt, t, setup, dudt=True)
        project_(dudt, setup, psolver, scalarfield(setup))
        ctx.u = tmp
        return dudt

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        φ = project_pullback_(_copy(s, g, True), s, ctx.psolver, scalarfield(s))
        O.apply_bc_u_pullback_(φ, 0.0, s, dudt=True)
        ubar = O.momentum_pullback_(vectorfield(s), φ, ctx.u, s)
        return O.apply_bc_u_pullback_(ubar, 0.0, s), None, None, None


def project(u, setup, psolver):
    """pressure.jl:52-82: u − G bc_p(poisson(Ω D u)); pullback φ − Dᵀ Ω poisson bc_pᵀ Gᵀ φ in one native sequence."""
    return _Project.apply(u, setup, psolver)


def right_hand_side(u, params, t):
    """sciml.jl:49-113: du/dt = project(bc(momentum(bc(u)))), `params = (setup, psolver)`."""
    setup, psolver = params[0], params[1]
    return _RightHandSide.apply(u, float(t), setup, psolver)


def create_right_hand_side(setup, psolver):
    """sciml.jl:13-19: `right_hand_side(u, param, t)`, differentiable in u."""

    def rhs(u, param, t):
        return right_hand_side(u, (setup, psolver), t)

    return rhs


# ------------------------------------------------------------------------------------ DNS-to-LES filters
class _Filter(torch.autograd.Function):
    """`v = Φ(u, setup_les, comp)` (lib/NeuralClosure filter.jl) with the exact transpose as backward (csrc/ins_filter.hip): a loss on
    filtered quantities of a differentiable DNS step.  `Filter.apply(u, setup_les, comp, setup_dns=None)`."""

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
        return cls._filter()(_field(dns, u, True), setup_les, int(comp), setup_dns=dns)

    @classmethod
    def backward(cls, ctx, g):
        ubar = cls._filter().pullback_(vectorfield(ctx.dns), _field(ctx.les, g, True), ctx.les, ctx.comp, ctx.dns)
        return ubar, None, None, None


class FaceAverage(_Filter):
    """filter.jl:26-46"""

    _kind = "face"


class VolumeAverage(_Filter):
    """filter.jl:82-116"""

    _kind = "volume"


# ------------------------------------------------------------------------------------ tensor-basis closure
def _nfield(setup, x, ncomp, fresh=False):
    """`x` as an N + (ncomp,) field in the library's layout (a copy when it has another one, or when `fresh`)."""
    from .setup import _alloc

    shape = tuple(setup.grid.N) + (ncomp,)
    if (not fresh and x.dtype == torch.float64 and x.device == setup.device and tuple(x.shape) == shape
            and tuple(x.stride()) == _fortran_strides(shape)):
        return x.detach()
    if tuple(x.shape) != shape:
        raise ValueError(f"expected a field of shape {shape}, got {tuple(x.shape)}")
    f = _alloc(setup, shape)
    f.copy_(x.detach())
    return f


def _check_f64(setup, *xs):
    for x in xs:
        if x.dtype != torch.float64:
            raise TypeError("fields must be float64 torch tensors")
        if x.device != setup.device:
            raise ValueError(f"field lives on {x.device}, setup on {setup.device}")


class _TensorBasis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        ctx.set_materialize_grads(False)
        _check_f64(setup, u)
        return O.tensorbasis(_saved_field(ctx, setup, u), setup)

    @staticmethod
    def backward(ctx, gB, gV):
        s = ctx.setup
        if gB is None and gV is None:
            return None, None
        D = s.grid.dimension
        nb, nv, _ = O._tb_sizes(s)
        Bbar = None if gB is None else _nfield(s, gB, nb * D * D)
        Vbar = None if gV is None else _nfield(s, gV, nv)
        return O.tensorbasis_pullback_(vectorfield(s), Bbar, Vbar, _saved(ctx), s), None


class _DivOfTensor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, σ, setup):
        ctx.setup = setup
        _check_f64(setup, σ)
        return O.divoftensor_(vectorfield(setup), _nfield(setup, σ, O._tb_sizes(setup)[2]), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.divoftensor_adjoint_(O.tensorfield(s), _field(s, g, True), s), None


class _TensorInvariants(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        from .setup import _alloc

        ctx.setup = setup
        _check_f64(setup, u)
        V = _alloc(setup, tuple(setup.grid.N) + (O._tb_sizes(setup)[1],))
        return O.tensorinvariants_(V, _saved_field(ctx, setup, u), setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        Vbar = _nfield(s, g, O._tb_sizes(s)[1])
        return O.tensorclosure_pullback_(vectorfield(s), None, None, Vbar, _saved(ctx), None, s), None


class _TensorClosureStress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, a, setup):
        ctx.setup = setup
        _check_f64(setup, u, a)
        uf = _field(setup, u, True)
        af = _nfield(setup, a, O._tb_sizes(setup)[0])
        # both inputs go through save_for_backward when they already are library fields: an in-place change before backward() raises
        ctx.ucopy = None if uf is u else uf
        ctx.acopy = None if af.data_ptr() == a.data_ptr() else af
        ctx.save_for_backward(*([u] if ctx.ucopy is None else []), *([a] if ctx.acopy is None else []))
        return O.tensorclosure_stress_(O.tensorfield(setup), uf, af, setup)

    @staticmethod
    def backward(ctx, g):
        from .setup import _alloc

        s = ctx.setup
        saved = list(ctx.saved_tensors)
        u = saved.pop(0) if ctx.ucopy is None else ctx.ucopy
        a = saved.pop(0).detach() if ctx.acopy is None else ctx.acopy
        nb, _, ns = O._tb_sizes(s)
        abar = _alloc(s, tuple(s.grid.N) + (nb,))
        ubar = O.tensorclosure_pullback_(vectorfield(s), abar, _nfield(s, g, ns), None, u, a, s)
        return ubar, abar, None


def tensorbasis(u, setup):
    """tensorbasis.jl:1-15 (rrule: tensorbasis_adjoint!, here in 2-D and 3-D): `(B, V)` as `ins_amd.tensorbasis`."""
    return _TensorBasis.apply(u, setup)


def divoftensor(σ, setup):
    """operators.jl:1155-1184 (rrule: divoftensor_adjoint!) on a symmetric `tensorfield` N + (D(D+1)/2,)."""
    return _DivOfTensor.apply(σ, setup)


def lastdimcontract(a, b):
    """tensorbasis.jl:97-157: c[I] = Σ_i a[I, i] b[I, i, ...] — plain torch (its pullback is torch's)."""
    return (a.reshape(a.shape + (1,) * (b.dim() - a.dim())) * b).sum(dim=a.dim() - 1)


def tensorinvariants(u, setup):
    """The invariants V of `tensorbasis` alone (N + (nv,), written on Ip), without forming B."""
    return _TensorInvariants.apply(u, setup)


def tensorclosure_stress(u, a, setup):
    """τ = Σ_i a_i B_i(u) as a symmetric `tensorfield` (written on Ip): `lastdimcontract(a, tensorbasis(u)[0])` in one kernel that keeps the
    basis in registers; the backward gives ubar and abar_i = <τbar, B_i>.  `a` is N + (nb,)."""
    return _TensorClosureStress.apply(u, a, setup)


def apply_bc_p_fields(σ, t, setup):
    """`apply_bc_p` on every channel of an N + (n,) field (the stress tensor's ghost fill, operators.jl:1296)."""
    return torch.stack([apply_bc_p(σ[..., q], t, setup) for q in range(σ.shape[-1])], dim=-1)


def _gridsize2(setup):
    """gridsize² = Σ_α Δ_α[I_α]² over the padded array (operators.jl:1137)."""
    g = setup.grid
    D = g.dimension
    d2 = torch.zeros(tuple(g.N), dtype=torch.float64, device=setup.device)
    for α in range(D):
        shape = [1] * D
        shape[α] = g.N[α]
        d2 = d2 + torch.as_tensor(np.asarray(g.Δ[α], dtype=np.float64) ** 2, device=setup.device).reshape(shape)
    return d2


def smagorinsky_closure(setup):
    """Differentiable Smagorinsky closure `m(u, θ)` (operators.jl:1284-1300), θ a 0-dim tensor: the member a_2 = 2 θ² d² sqrt(2 V_1), every
    other a_i = 0, of the tensor-basis family, so ∂/∂u runs in the fused kernels and ∂/∂θ is torch's: a learnable Smagorinsky constant."""
    g = setup.grid
    D = g.dimension
    nb = O._tb_sizes(setup)[0]
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    pads = [q for α in reversed(range(D)) for q in (g.Ip[α][0], g.N[α] - g.Ip[α][1])]
    d2 = _gridsize2(setup)[ip]

    def closure(u, θ):
        θ = torch.as_tensor(θ, dtype=torch.float64, device=setup.device)
        V = tensorinvariants(u, setup)
        a2 = torch.nn.functional.pad(2 * θ * θ * d2 * torch.sqrt(2 * V[ip + (0,)]), pads)  # Ip only: sqrt has no derivative at the zeros outside
        z = torch.zeros_like(a2)
        a = torch.stack([z, a2] + [z] * (nb - 2), dim=-1)
        τ = apply_bc_p_fields(tensorclosure_stress(u, a, setup), 0.0, setup)
        return divoftensor(τ, setup)

    return closure


# ------------------------------------------------------------------------------------ time stepping
def timestep(method, stepper, Δt, θ=None):
    """step_explicit_runge_kutta.jl:61-120: one explicit Runge-Kutta step without mutation, differentiable in `stepper.u`, in `stepper.temp`
    (with the temperature equation) and (through a torch closure model `m(u, θ)`) in θ.  The stage combinations are torch arithmetic; with a
    temperature field the right-hand side of a stage, (u, temp) -> (F, Ftemp), is one Function whose backward is two launches."""
    setup, psolver, u, temp, t, n = stepper.setup, stepper.psolver, stepper.u, stepper.temp, stepper.t, stepper.n
    if temp is not None and setup.temperature is None:
        raise ValueError("a temperature field needs setup.temperature (temperature_equation)")
    m = setup.closure_model
    if m is not None and getattr(m, "_ins_closure", None) == "smagorinsky" and torch.is_grad_enabled():
        raise NotImplementedError("ad.timestep: the Smagorinsky closure has no pullback; give the closure as a torch function m(u, θ)")
    tempplanes = temp is not None and any(isinstance(bc, DirichletBC) and callable(bc.u) for side in setup.temperature.boundary_conditions for bc in side)
    if isinstance(method, LMWray3) and (setup.needs_bc_planes or tempplanes or (setup.bodyforce is not None and not setup.issteadybodyforce)):
        # the native step runs the low-storage loop then (step_lmwray3.jl), whose ghost fills happen at other times than the ERK form's
        raise NotImplementedError("ad.timestep: LMWray3 with time-dependent boundary data or body force; use an ExplicitRungeKuttaMethod")
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    A, c = erk.A, erk.c
    tstart, ustart, tempstart, ku, ktemp = t, u, temp, [], []
    for i in range(len(erk.b)):
        u = apply_bc_u(u, t, setup)
        if temp is None:
            F = momentum(u, None, t, setup)
        else:
            temp = apply_bc_temp(temp, t, setup)
            F, Ftemp = _StageRightHandSide.apply(u, temp, t, setup)
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


# ------------------------------------------------------------------------------------ checkpointed rollouts
class _StepAdjoint:
    """`ins_rk_adjoint_t` (csrc/ins_rk_adjoint.hip): the work arrays of the native reverse step, with the forward's native cache beside it."""

    def __init__(self, erk, setup, psolver):
        import ctypes as C

        from . import _lib
        from .time_steppers import ERKCache

        self.erk, self.setup, self.cache = erk, setup, ERKCache(erk, setup, psolver)
        A = np.ascontiguousarray(erk.A, dtype=np.float64)
        c = np.ascontiguousarray(erk.c, dtype=np.float64)
        self._handle = C.c_void_p()
        _lib.call("ins_rk_adjoint_create", setup.handle, psolver.handle, len(erk.b), A.ctypes.data_as(_lib.c_double_p), c.ctypes.data_as(_lib.c_double_p),
                  C.byref(self._handle))

    def step_pullback_(self, ubar, ustart, Δt):
        """ubar: ∂L/∂u_out -> ∂L/∂ustart, in place: the whole reverse sweep of one step is this one call."""
        from . import _lib

        setup = self.setup
        f = setup.bodyforce if (setup.bodyforce is not None and setup.issteadybodyforce) else None
        _lib.call("ins_rk_step_pullback_f64", self._handle, 1.0 / setup.Re, setup.ptr(ustart, True), setup.ptr(f, True) if f is not None else None, float(Δt),
                  setup.ptr(ubar, True), setup.stream)
        return ubar

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                from . import _lib

                _lib.load().ins_rk_adjoint_destroy(h)
            except Exception:
                pass


def _step_adjoint(erk, setup, psolver):
    """One `_StepAdjoint` per (solver, tableau), kept on the solver."""
    key = (np.asarray(erk.A, dtype=np.float64).tobytes(), np.asarray(erk.c, dtype=np.float64).tobytes())
    store = psolver.__dict__.setdefault("_ad_step_adjoints", {})
    if key not in store:
        store[key] = _StepAdjoint(erk, setup, psolver)
    return store[key]


def _native_steps_(adj, u, t, Δt, nsteps):
    """`nsteps` native steps on `u`, in place (`timesteps_` = ins_rk_steps_f64; one step: ins_rk_step_f64)."""
    from .time_steppers import timesteps_

    setup, cache = adj.setup, adj.cache
    timesteps_(adj.erk, create_stepper(adj.erk, setup=setup, psolver=cache.psolver, u=u, t=t), Δt, nsteps, cache=cache)
    return u


class _TimeSteps(torch.autograd.Function):
    """u -> u after nsteps Runge-Kutta steps.  Saved: the state at the start of every chunk of `every` steps, nothing else."""

    @staticmethod
    def forward(ctx, u, adj, t, Δt, nsteps, every):
        setup = adj.setup
        out = _copy(setup, u, True)
        ctx.adj, ctx.t, ctx.Δt, ctx.nsteps, ctx.every = adj, t, Δt, nsteps, every
        ctx.checkpoints = []
        for start in range(0, nsteps, every):
            ctx.checkpoints.append(_copy(setup, out, True))
            _native_steps_(adj, out, t + start * Δt, Δt, min(every, nsteps - start))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from .time_steppers import combine_

        adj, Δt, nsteps, every = ctx.adj, ctx.Δt, ctx.nsteps, ctx.every
        setup = adj.setup
        ubar = _copy(setup, g, True)
        bufs = [vectorfield(setup) for _ in range(min(every, nsteps) - 1)]  # the step-start states of one chunk after its checkpoint
        starts = list(range(0, nsteps, every))
        for q in reversed(range(len(starts))):
            n = min(every, nsteps - starts[q])
            states = [ctx.checkpoints[q]]
            for j in range(1, n):
                combine_(bufs[j - 1], states[j - 1], [], [], setup)  # a copy by the library's own pass
                states.append(_native_steps_(adj, bufs[j - 1], ctx.t + (starts[q] + j - 1) * Δt, Δt, 1))
            for j in reversed(range(n)):
                adj.step_pullback_(ubar, states[j], Δt)
            ctx.checkpoints[q] = None
        return ubar, None, None, None, None, None


def timesteps(method, stepper, Δt, nsteps, *, checkpoint_every=None):
    """`nsteps` calls of `ad.timestep(method, ·, Δt)` as one Function: nothing is mutated, the result is differentiable in `stepper.u`.

    The forward is the native multi-step loop (`timesteps_`, ins_rk_steps_f64) in chunks of `checkpoint_every` steps (default ceil(sqrt(nsteps)));
    only the state at the start of every chunk is kept.  The backward walks the chunks in reverse: it recomputes the chunk's step-start states with the
    native step and calls the native step pullback (ins_rk_step_pullback_f64) once per step.  Memory: ceil(nsteps/c) + c - 1 vector fields and the
    2s + 1 work arrays of the reverse step, instead of the unrolled graph's ~10 fields per stage.

    Scope: what the native isothermal loop runs — fp64, ExplicitRungeKuttaMethod or LMWray3, 2-D / 3-D, any boundary conditions with constant data, any
    solver, no body force or a steady one.  Anything else raises NotImplementedError: use `ad.timestep` step by step."""
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError(f"ad.timesteps: nsteps must be >= 1, got {nsteps}")
    every = int(np.ceil(np.sqrt(nsteps))) if checkpoint_every is None else int(checkpoint_every)
    if every < 1:
        raise ValueError(f"ad.timesteps: checkpoint_every must be >= 1, got {checkpoint_every}")
    setup, psolver, u = stepper.setup, stepper.psolver, stepper.u
    if u.dtype != torch.float64:
        raise TypeError("ad.timesteps: fields must be float64 torch tensors (the Float32 family has ad32.timestep)")
    from .boundary_conditions import HaloBC

    if setup.closure_model is not None:
        raise NotImplementedError("ad.timesteps: a closure model is not part of the native reverse loop; use ad.timestep step by step")
    if stepper.temp is not None or setup.temperature is not None:
        raise NotImplementedError("ad.timesteps: the temperature equation is not part of the native reverse loop; use ad.timestep step by step")
    if setup.needs_bc_planes:
        raise NotImplementedError("ad.timesteps: callable Dirichlet data needs the host between the stages; use ad.timestep step by step")
    if setup.bodyforce is not None and not setup.issteadybodyforce:
        raise NotImplementedError("ad.timesteps: an unsteady body force is evaluated on the host; use ad.timestep step by step")
    if any(isinstance(bc, HaloBC) for side in setup.boundary_conditions for bc in side):
        raise NotImplementedError("ad.timesteps: slab (halo) setups are not supported; use ad.timestep step by step")
    _check_f64(setup, u)
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    adj = _step_adjoint(erk, setup, psolver)
    t = float(stepper.t)
    if torch.is_grad_enabled() and u.requires_grad:
        out = _TimeSteps.apply(u, adj, t, float(Δt), nsteps, min(every, nsteps))
    else:  # nothing to save: one native call
        out = _native_steps_(adj, _copy(setup, u, True), t, float(Δt), nsteps)
    return create_stepper(method, setup=setup, psolver=psolver, u=out, temp=None, t=t + nsteps * erk.c[-1] * Δt, n=stepper.n + nsteps)
