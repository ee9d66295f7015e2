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
from functools import partial
from types import SimpleNamespace

import numpy as np
import torch

from . import _autodiff_core as core
from . import operators as O
from ._step_route import Closure, Force, classify, steady_force
from .pressure import project_, project_pullback_
from .setup import _alloc, scalarfield, vectorfield
from .time_steppers import _PER_TRAJECTORY, LMWray3, _lmwray3_as_erk, create_stepper

__all__ = ["apply_bc_u", "apply_bc_p", "apply_bc_temp", "gravity", "convection_diffusion_temp", "dissipation", "scalewithvolume", "divergence", "pressuregradient", "applypressure", "poisson", "convection", "diffusion",
           "momentum", "project", "right_hand_side", "create_right_hand_side", "timestep", "timesteps", "FaceAverage", "VolumeAverage", "tensorbasis", "divoftensor",
           "lastdimcontract", "tensorinvariants", "tensorclosure_stress", "apply_bc_p_fields", "smagorinsky_closure", "smagorinsky_force",
           "ensemble_apply_bc_u", "ensemble_momentum", "ensemble_project", "timestep_ensemble"]


def _check_f64(setup, *xs):
    for x in xs:
        if x.dtype != torch.float64:
            raise TypeError("fields must be float64 torch tensors")
        if x.device != setup.device:
            raise ValueError(f"field lives on {x.device}, setup on {setup.device}")


def _rk_adjoint_create(erk, setup, psolver):
    """`ins_rk_adjoint_t` (csrc/ins_rk_adjoint.hip): the work arrays of the native reverse step."""
    import ctypes as C

    from . import _lib

    A = np.ascontiguousarray(erk.A, dtype=np.float64)
    c = np.ascontiguousarray(erk.c, dtype=np.float64)
    handle = C.c_void_p()
    _lib.call("ins_rk_adjoint_create", setup.handle, psolver.handle, len(erk.b), A.ctypes.data_as(_lib.c_double_p), c.ctypes.data_as(_lib.c_double_p),
              C.byref(handle))
    return handle


def _rk_adjoint_destroy(handle):
    from . import _lib

    _lib.load().ins_rk_adjoint_destroy(handle)


def _rk_cache(erk, setup, psolver):
    from .time_steppers import ERKCache

    return ERKCache(erk, setup, psolver)


def _rk_steps_(adj, u, temp, t, Δt, nsteps, θ=None):
    """`timesteps_`: ins_rk_steps_f64, or with a temperature or the Smagorinsky closure (θ) ins_rk_step_ext_f64 step by step."""
    from .time_steppers import timesteps_

    with core.native_closure(adj.setup, θ, O.smagorinsky_closure):
        timesteps_(adj.erk, create_stepper(adj.erk, setup=adj.setup, psolver=adj.cache.psolver, u=u, temp=temp, t=t), Δt, nsteps, θ=θ, cache=adj.cache)


def _rk_adjoint_set_closure(adj, θ, θbar):
    """ins_rk_adjoint_set_closure: kind 1 with θ and the device double of `θbar`, or kind 0."""
    from . import _lib

    if θ is None:
        _lib.call("ins_rk_adjoint_set_closure", adj._handle, 0, 0.0, None)
    else:
        _lib.call("ins_rk_adjoint_set_closure", adj._handle, 1, float(θ), O._thetabar_ptr(adj.setup, θbar))


def _rk_step_pullback_(adj, ubar, tempbar, ustart, tempstart, Δt):
    """ins_rk_step_pullback_f64, with a temperature ins_rk_step_pullback_ext_f64 (the descriptor goes to the handle with every call)."""
    import ctypes as C

    from . import _lib
    from .time_steppers import _temperature_desc

    setup = adj.setup
    f = steady_force(setup)
    fp = setup.ptr(f, True) if f is not None else None
    if tempbar is None:
        _lib.call("ins_rk_step_pullback_f64", adj._handle, 1.0 / setup.Re, setup.ptr(ustart, True), fp, float(Δt), setup.ptr(ubar, True), setup.stream)
        return
    desc = _temperature_desc(setup)  # per call, like the forward: `setup.temperature` may have been replaced since the last one
    _lib.call("ins_rk_adjoint_set_temperature", adj._handle, C.byref(desc))
    _lib.call("ins_rk_step_pullback_ext_f64", adj._handle, 1.0 / setup.Re, setup.ptr(ustart, True), setup.ptr(tempstart, False), fp, float(Δt),
              setup.ptr(ubar, True), setup.ptr(tempbar, False), setup.stream)


def _rk_copy_(dst, src, setup, vector):
    """a copy by the library's own pass"""
    from .time_steppers import combine_

    return combine_(dst, src, [], [], setup, vector=vector)


# The fp64 precision table of the shared autograd layer (_autodiff_core.py): `operators.py` under the table's calling conventions.  Other dtypes
# are converted silently, except by the tensor-basis Functions (`_check_f64`); the body force is inside `O.momentum_` and may depend on `t`; the
# pullbacks of the ghost fills take a time that does not enter (0.0).
_OPS = SimpleNamespace(
    name="ad", dtype=torch.float64,
    scalarfield=scalarfield, vectorfield=vectorfield, nfield=lambda setup, ncomp: _alloc(setup, tuple(setup.grid.N) + (ncomp,)),
    tensorfield=O.tensorfield, tb_sizes=O._tb_sizes,
    check_dtype=lambda x: None,
    check_closure_inputs=lambda setup, u, *others: _check_f64(setup, *(() if u is None else (u,)), *others),
    bodyforce=lambda setup: None,
    apply_bc_u_=lambda u, t, setup, dudt: O.apply_bc_u_(u, t, setup, dudt=dudt),
    apply_bc_p_=O.apply_bc_p_, apply_bc_temp_=O.apply_bc_temp_, momentum_=O.momentum_, gravity_=O.gravity_,
    convection_diffusion_temp_=O.convection_diffusion_temp_, dissipation_=O.dissipation_, project_=project_, divoftensor_=O.divoftensor_,
    tensorinvariants_=O.tensorinvariants_, tensorclosure_stress_=O.tensorclosure_stress_,
    apply_bc_u_pullback_=lambda φbar, setup: O.apply_bc_u_pullback_(φbar, 0.0, setup),
    apply_bc_p_pullback_=lambda φbar, setup: O.apply_bc_p_pullback_(φbar, 0.0, setup),
    apply_bc_temp_pullback_=lambda tempbar, setup: O.apply_bc_temp_pullback_(tempbar, 0.0, setup),
    momentum_pullback_=O.momentum_pullback_, gravity_adjoint_=O.gravity_adjoint_,
    convection_diffusion_temp_adjoint_=O.convection_diffusion_temp_adjoint_, dissipation_adjoint_=O.dissipation_adjoint_,
    temperature_pullback_=O.temperature_pullback_, project_pullback_=project_pullback_, divoftensor_adjoint_=O.divoftensor_adjoint_,
    tensorclosure_pullback_=O.tensorclosure_pullback_,
    smagorinsky_force_=O.smagorinsky_force_,
    smagorinsky_force_pullback_=lambda ubar, θbar, sbar, u, θ, setup: O.smagorinsky_force_pullback_(ubar, θbar, sbar, u, θ, setup),
    rk_adjoint_set_closure=_rk_adjoint_set_closure,
    rk_cache=_rk_cache, rk_adjoint_create=_rk_adjoint_create, rk_adjoint_destroy=_rk_adjoint_destroy, rk_steps_=_rk_steps_,
    rk_step_pullback_=_rk_step_pullback_, rk_copy_=_rk_copy_,
)
# the shared helpers, for the fp64-only Functions below
_field, _copy, _save_inputs, _saved_inputs = partial(core._field, _OPS), partial(core._copy, _OPS), partial(core._save_inputs, _OPS), core._saved_inputs
# private names the tests reach for, under their fp64 spelling
_gridsize2 = core._gridsize2
_StageRightHandSide = SimpleNamespace(apply=lambda u, temp, t, setup: core._StageRightHandSide.apply(u, temp, t, setup, _OPS))
_step_adjoint = partial(core._step_adjoint, _OPS)


# ------------------------------------------------------------------------------------ ghost fill
def apply_bc_u(u, t, setup, dudt=False):
    """boundary_conditions.jl:114-167 (rrule: apply_bc_u_pullback!)"""
    return core._ApplyBCU.apply(u, t, setup, bool(dudt), _OPS)


def apply_bc_p(p, t, setup):
    """boundary_conditions.jl:114-206 (rrule: apply_bc_p_pullback!)"""
    return core._ApplyBCP.apply(p, t, setup, _OPS)


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
        (uf,) = _save_inputs(ctx, setup, [(u, True)])
        return O.convection(uf, setup)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        (u,) = _saved_inputs(ctx)
        return O.convection_adjoint_(vectorfield(s), _field(s, g, True), u, s), None


class _Diffusion(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, use_viscosity):
        ctx.setup, ctx.use_viscosity = setup, use_viscosity
        return O.diffusion(_field(setup, u, True), setup, use_viscosity)

    @staticmethod
    def backward(ctx, g):
        s = ctx.setup
        return O.diffusion_adjoint_(vectorfield(s), _field(s, g, True), s, ctx.use_viscosity), None, None


def convection(u, setup):
    """operators.jl:366-415 (rrule: convection_adjoint!)"""
    return _Convection.apply(u, setup)


def diffusion(u, setup, use_viscosity=True):
    """operators.jl:521-573 (rrule: diffusion_adjoint!)"""
    return _Diffusion.apply(u, setup, bool(use_viscosity))


def momentum(u, temp, t, setup):
    """operators.jl:940-976 (convection + diffusion + body force; the pullback is one fused kernel).  With a temperature field the gravity term
    is added (operators.jl:974), differentiable in `u` and in `temp`."""
    if temp is not None and setup.temperature is None:
        raise NotImplementedError("ad.momentum: a temperature field needs setup.temperature (temperature_equation)")
    return core.momentum(_OPS, u, temp, t, setup)


# ------------------------------------------------------------------------------------ temperature equation
def _need_temperature(setup, what):
    if setup.temperature is None:
        raise ValueError(f"ad.{what} needs setup.temperature (temperature_equation)")


def apply_bc_temp(temp, t, setup):
    """boundary_conditions.jl:236-246 (rrule: apply_bc_temp_pullback!)"""
    _need_temperature(setup, "apply_bc_temp")
    return core._ApplyBCTemp.apply(temp, t, setup, _OPS)


def gravity(temp, setup):
    """operators.jl:884-931 (rrule: gravity_adjoint!)"""
    _need_temperature(setup, "gravity")
    return core._Gravity.apply(temp, setup, _OPS)


def convection_diffusion_temp(u, temp, setup):
    """operators.jl:692-737, differentiable in `u` and in `temp` (the reference's rrule, :699-704, returns undefined names)."""
    _need_temperature(setup, "convection_diffusion_temp")
    return core._ConvectionDiffusionTemp.apply(u, temp, setup, _OPS)


def dissipation(u, setup):
    """operators.jl:770-814 (the reference's rrule is @test_broken); the pullback recomputes diffusion(u) in the kernel."""
    _need_temperature(setup, "dissipation")
    return core._Dissipation.apply(u, setup, _OPS)


# ------------------------------------------------------------------------------------ projection and right-hand side
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
    return core._Project.apply(u, setup, psolver, _OPS)


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
# `v = Φ(u, setup_les, comp)` (lib/NeuralClosure filter.jl) with the exact transpose as backward (csrc/ins_filter.hip): a loss on filtered
# quantities of a differentiable DNS step.  `Filter.apply(u, setup_les, comp, setup_dns=None)`.
FaceAverage = core.filter_function("FaceAverage", _OPS, "filter.jl:26-46")
VolumeAverage = core.filter_function("VolumeAverage", _OPS, "filter.jl:82-116")


# ------------------------------------------------------------------------------------ tensor-basis closure
class _TensorBasis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup):
        ctx.setup = setup
        ctx.set_materialize_grads(False)
        _check_f64(setup, u)
        (uf,) = _save_inputs(ctx, setup, [(u, True)])
        return O.tensorbasis(uf, setup)

    @staticmethod
    def backward(ctx, gB, gV):
        s = ctx.setup
        if gB is None and gV is None:
            return None, None
        D = s.grid.dimension
        nb, nv, _ = O._tb_sizes(s)
        Bbar = None if gB is None else _field(s, gB, nb * D * D)
        Vbar = None if gV is None else _field(s, gV, nv)
        (u,) = _saved_inputs(ctx)
        return O.tensorbasis_pullback_(vectorfield(s), Bbar, Vbar, u, s), None


def tensorbasis(u, setup):
    """tensorbasis.jl:1-15 (rrule: tensorbasis_adjoint!, here in 2-D and 3-D): `(B, V)` as `ins_amd.tensorbasis`."""
    return _TensorBasis.apply(u, setup)


def divoftensor(σ, setup):
    """operators.jl:1155-1184 (rrule: divoftensor_adjoint!) on a symmetric `tensorfield` N + (D(D+1)/2,)."""
    return core._DivOfTensor.apply(σ, setup, _OPS)


lastdimcontract = core.lastdimcontract  # tensorbasis.jl:97-157


def tensorinvariants(u, setup):
    """The invariants V of `tensorbasis` alone (N + (nv,), written on Ip), without forming B."""
    return core._TensorInvariants.apply(u, setup, _OPS)


def tensorclosure_stress(u, a, setup):
    """τ = Σ_i a_i B_i(u) as a symmetric `tensorfield` (written on Ip): `lastdimcontract(a, tensorbasis(u)[0])` in one kernel that keeps the
    basis in registers; the backward gives ubar and abar_i = <τbar, B_i>.  `a` is N + (nb,)."""
    return core._TensorClosureStress.apply(u, a, setup, _OPS)


def apply_bc_p_fields(σ, t, setup):
    """`apply_bc_p` on every channel of an N + (n,) field (the stress tensor's ghost fill, operators.jl:1296)."""
    return core.apply_bc_p_fields(apply_bc_p, σ, t, setup)


def smagorinsky_closure(setup):
    """Differentiable Smagorinsky closure `m(u, θ)` (operators.jl:1284-1300), θ a 0-dim tensor: the member a_2 = 2 θ² d² sqrt(2 V_1), every
    other a_i = 0, of the tensor-basis family, so ∂/∂u runs in the fused kernels and ∂/∂θ is torch's: a learnable Smagorinsky constant."""
    return core.smagorinsky_closure(_OPS, setup)


def smagorinsky_force(u, θ, setup):
    """The Smagorinsky closure force `smagorinsky_closure(setup)(u, θ)` of a ghost-filled `u` (operators.jl:1284-1300) as ONE native call, with the
    fused pullback as backward (csrc/ins_smagpullback_kernels.h): ubar, and for a 0-dim tensor θ that requires grad θbar = 2θ <σ̄, σ̂>, which falls
    out of the same pass.  The same function of (u, θ) as `ad.smagorinsky_closure(setup)`, without its per-stage tensor-basis fields."""
    if classify(setup).slab:
        raise NotImplementedError("ad.smagorinsky_force: slab (halo) setups are not supported")
    return core.smagorinsky_force(_OPS, u, θ, setup)


# ------------------------------------------------------------------------------------ time stepping
def timestep(method, stepper, Δt, θ=None):
    """step_explicit_runge_kutta.jl:61-120: one explicit Runge-Kutta step without mutation, differentiable in `stepper.u`, in `stepper.temp`
    (with the temperature equation) and (through a torch closure model `m(u, θ)`) in θ.  The stage combinations are torch arithmetic; with a
    temperature field the right-hand side of a stage, (u, temp) -> (F, Ftemp), is one Function whose backward is two launches."""
    setup, temp = stepper.setup, stepper.temp
    if temp is not None and setup.temperature is None:
        raise ValueError("a temperature field needs setup.temperature (temperature_equation)")
    facts = classify(setup, temp, θ)
    if facts.closure is Closure.LIBRARY and torch.is_grad_enabled():
        raise NotImplementedError("ad.timestep: the Smagorinsky closure has no pullback; give the closure as a torch function m(u, θ)")
    if isinstance(method, LMWray3) and (facts.bc_u_callable or (facts.has_temp and facts.bc_temp_callable) or facts.force is Force.UNSTEADY):
        # the native step runs the low-storage loop then (step_lmwray3.jl), whose ghost fills happen at other times than the ERK form's
        raise NotImplementedError("ad.timestep: LMWray3 with time-dependent boundary data or body force; use an ExplicitRungeKuttaMethod")
    return core.timestep(_OPS, method, stepper, Δt, θ)


# ------------------------------------------------------------------------------------ B trajectories in one graph
def _ensemble_cache(cache, U, what):
    """The checks the member Functions share: an `EnsembleCache` (whose constructor has refused everything outside fp64 / 2-D / all-periodic / uniform /
    power-of-two sides / psolver_spectral / no body force, closure or temperature on the setup) and a float64 tensor of its shape."""
    from .time_steppers import EnsembleCache

    if not isinstance(cache, EnsembleCache):
        raise TypeError(f"ad.{what} needs an EnsembleCache (EnsembleCache(method, setup, psolver, B)); without one, {_PER_TRAJECTORY}")
    if not isinstance(U, torch.Tensor):
        raise TypeError(f"ad.{what}: ensemble fields are torch tensors (vectorfields)")
    if U.dtype == torch.float32:
        raise NotImplementedError(f"ad.{what}: Float32 ensembles are outside the member operators (fp64 only); {_PER_TRAJECTORY.replace('ad.', 'ad32.')}")
    shape = (cache.B,) + tuple(cache.setup.grid.N) + (2,)
    if tuple(U.shape) != shape:
        raise ValueError(f"ad.{what}: ensemble field must have shape {shape} (use vectorfields), got {tuple(U.shape)}")
    return cache


def ensemble_apply_bc_u(cache, U):
    """`ad.apply_bc_u` of every member of `U`, `(B,) + N + (2,)` as `vectorfields` makes it, in two launches forward and two backward."""
    return core._EnsembleApplyBCU.apply(U, _ensemble_cache(cache, U, "ensemble_apply_bc_u"))


def ensemble_momentum(cache, U):
    """`ad.momentum(U[b], None, t, setup)` of every member in one launch; the backward is the member form of the tiled momentum pullback
    (csrc/ins_adjoint.hip, k_momentum_pullback_members_2d), one launch.  `U` has valid ghost volumes."""
    return core._EnsembleMomentum.apply(U, _ensemble_cache(cache, U, "ensemble_momentum"))


def ensemble_project(cache, U):
    """`ad.apply_bc_u(ad.project(ad.apply_bc_u(U[b])))` of every member: the member solve and the gradient-subtract + ghost pass forward, and backward
    the ghost fold, the same solve and the gradient-subtract that leaves zero ghosts (the forward is E·P·R with P symmetric)."""
    return core._EnsembleProject.apply(U, _ensemble_cache(cache, U, "ensemble_project"))


def timestep_ensemble(method, cache, U, t, Δt, θ=None, closure=None):
    """One explicit Runge-Kutta step of all B members of `U` without mutation: `ad.timestep` of every trajectory as ONE autograd graph.  The launch count
    of the step's own operators and of their pullbacks does not depend on B; what `closure` launches is the closure's own (torch convolves float64
    tensors sample by sample: `neuralclosure.cnn(..., batched=True)` does not).  Returns the new `(B,) + N + (2,)` field (ghost volumes valid), differentiable in `U` and, through the torch member closure
    `closure(U, θ)` (`neuralclosure.wrappedclosure_ensemble`), in θ.  `t` is accepted for symmetry with `ad.timestep`: nothing in the scope depends on
    time.  `method`: an ExplicitRungeKuttaMethod with more than one stage, or LMWray3 (run as the explicit method it is).

    Scope: that of `EnsembleCache` — fp64, 2-D, all-periodic, exactly uniform, power-of-two sides 16 … 1024, `psolver_spectral`, no body force, no
    temperature, one Δt and Re for all members.  Everything else raises NotImplementedError naming `ad.timestep` per trajectory."""
    _ensemble_cache(cache, U, "timestep_ensemble")
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    if len(erk.b) < 2:
        raise NotImplementedError(f"ad.timestep_ensemble: a one-stage method is outside the ensemble loop; {_PER_TRAJECTORY}")
    return core.timestep_ensemble(erk, cache, U, float(Δt), θ, closure)


# ------------------------------------------------------------------------------------ checkpointed rollouts
def timesteps(method, stepper, Δt, nsteps, *, θ=None, checkpoint_every=None):
    """`nsteps` calls of `ad.timestep(method, ·, Δt)` as one Function: nothing is mutated, the result is differentiable in `stepper.u`, with
    the temperature equation in `stepper.temp`, and with the Smagorinsky closure in its constant θ.

    With `setup.closure_model` the library's Smagorinsky closure of this setup (`ins.smagorinsky_closure(setup)` or `ad.smagorinsky_closure(setup)`)
    and `θ` its constant (a Python scalar, or a 0-dim tensor that may require grad) the closure runs inside both native loops: the forward is
    `timesteps_(…, θ=float(θ))`, the reverse step recomputes k_i = F(v_i) [+ gravity] + f + m(v_i, θ) and adds the closure's fused pullback
    (ins_smagorinsky_force_pullback_f64) to every stage; ∂L/∂θ of all steps and chunks is summed in one device double.  The handle then holds one
    vector field more, and the grid handle the D·D fields of ∇ubar.

    The forward is the native multi-step loop (`timesteps_`: ins_rk_steps_f64, with a temperature ins_rk_step_ext_f64 per step) in chunks of
    `checkpoint_every` steps (default ceil(sqrt(nsteps))); only the state at the start of every chunk is kept.  The backward walks the chunks in
    reverse: it recomputes the chunk's step-start states with the native step and calls the native step pullback (ins_rk_step_pullback_f64, with
    a temperature ins_rk_step_pullback_ext_f64) once per step.  Memory: ceil(nsteps/c) + c - 1 states and the work arrays of the reverse step
    (2s + 1 vector fields, with a temperature 2s + 1 scalar fields more), instead of the unrolled graph's ~10 fields per stage.

    Scope: fp64, ExplicitRungeKuttaMethod or LMWray3, 2-D / 3-D, any boundary conditions with constant data for u and for temp, any solver, no
    body force or a steady one, with or without `setup.temperature`.  Any other closure model, a Smagorinsky closure without θ, θ without a closure,
    callable boundary data, an unsteady body force and slab setups raise NotImplementedError: use `ad.timestep` step by step.  Float32 fields:
    `ad32.timesteps`."""
    nsteps, every = core.checkpoint_interval(_OPS, nsteps, checkpoint_every)
    setup, u, temp = stepper.setup, stepper.u, stepper.temp
    core.check_rollout(_OPS, stepper, θ)
    _check_f64(setup, u, *(() if temp is None else (temp,)))
    return core.timesteps(_OPS, method, stepper, Δt, nsteps, every, θ=θ)
