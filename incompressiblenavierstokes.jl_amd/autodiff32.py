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
from types import SimpleNamespace

import torch

from . import _autodiff_core as core
from . import f32 as F32
from ._step_route import Closure, Force, classify
from .boundary_conditions import PeriodicBC

__all__ = ["apply_bc_u", "momentum", "project", "timestep"]  # `timesteps` and the operators below are module attributes (an existing test pins this list)


def _check_slab(setup, what):
    facts = classify(setup)
    if facts.slab:
        raise NotImplementedError(f"ad32.{what}: slab (halo) setups run in fp64 only")
    return facts


def _check_setup(setup, what):
    facts = _check_slab(setup, what)
    if facts.bc_u_callable:
        raise NotImplementedError(f"ad32.{what}: the _f32 family takes constant boundary data (callable DirichletBC values: use ins_amd.ad)")
    if facts.force is Force.UNSTEADY:
        raise NotImplementedError(f"ad32.{what}: an unsteady body force is evaluated in fp64 on the host (use ins_amd.ad)")
    if facts.closure is Closure.LIBRARY:
        raise NotImplementedError(f"ad32.{what}: the fused Smagorinsky closure is fp64 and has no pullback; use ad32.smagorinsky_closure(setup), "
                                  "or give the closure as a torch function m(u, θ)")


def _check_psolver(setup, psolver, what):
    from .pressure import psolver_spectral

    if not isinstance(psolver, F32.psolver_spectral32):
        raise TypeError(f"ad32.{what} takes a Float32 pressure solver (f32.psolver_spectral32, f32.psolver_wrap32, f32.default_psolver32)")
    inner = getattr(psolver, "psolver64", None)
    if isinstance(inner, psolver_spectral) and all(isinstance(bc, PeriodicBC) for side in setup.boundary_conditions for bc in side):
        raise NotImplementedError(f"ad32.{what}: psolver_wrap32 around psolver_spectral on an all-periodic box is not taken; use f32.psolver_spectral32")


def _periodic_uniform(setup):
    """The boxes on which the Float32 family runs its periodic kernels: the classification of `default_psolver` (pressure.jl:85-98)."""
    import math

    import numpy as np

    if not all(isinstance(bc, PeriodicBC) for side in setup.boundary_conditions for bc in side):
        return False
    return all(np.allclose(d, d[0], rtol=math.sqrt(np.finfo(np.float64).eps), atol=0) for d in setup.grid.Δ)


def _check_temperature(setup, what):
    _check_slab(setup, what)
    if setup.temperature is None:
        raise ValueError(f"ad32.{what} needs setup.temperature (temperature_equation)")


def _check_dtype(x):
    if x.dtype != torch.float32:
        raise TypeError("ad32 takes float32 torch tensors")


def _check_vec(setup, u, *others):
    """`u` is a float32 vector field of the setup's shape: another dtype raises TypeError, another shape ValueError (the N + (n,) inputs are
    checked where they are converted)."""
    if u is not None:
        shape = tuple(setup.grid.N) + (setup.grid.dimension,)
        _check_dtype(u)
        if tuple(u.shape) != shape:
            raise ValueError(f"expected a field of shape {shape}, got {tuple(u.shape)}")


def _bodyforce32(setup):
    f = getattr(setup, "_bodyforce32", None)
    if f is None or f[0] is not setup.bodyforce:
        f = (setup.bodyforce, F32.to_f32(setup, setup.bodyforce))
        setup._bodyforce32 = f
    return f[1]


def _rk_adjoint_create(erk, setup, psolver):
    """`ins_rk_adjoint32_t` (csrc/ins_rk_adjoint.hip): the float work arrays of the native reverse step."""
    import ctypes as C

    import numpy as np

    from . import _lib

    A = np.ascontiguousarray(erk.A, dtype=np.float64)
    c = np.ascontiguousarray(erk.c, dtype=np.float64)
    handle = C.c_void_p()
    _lib.call("ins_rk_adjoint_create_f32", setup.handle, psolver.handle, len(erk.b), A.ctypes.data_as(_lib.c_double_p), c.ctypes.data_as(_lib.c_double_p),
              C.byref(handle))
    return handle


def _rk_adjoint_destroy(handle):
    from . import _lib

    _lib.load().ins_rk_adjoint_destroy_f32(handle)


def _rk_cache(erk, setup, psolver):
    """The forward's native cache.  `ERKCache32` keeps its solver alive, which is right for a cache a caller holds (the native handle borrows the
    solver), but this one is kept ON the solver (`_step_adjoint`), which therefore outlives it anyway: it refers to the solver weakly, so there is no
    reference cycle and solver, reverse-step handle and cache (and the solver's hipFFT plans) go by reference count, not at some later garbage
    collection."""
    import weakref

    cache = F32.ERKCache32(erk, setup, psolver)
    cache.psolver = weakref.proxy(psolver)
    return cache


def _rk_steps_(adj, u, temp, t, Δt, nsteps, θ=None):
    """`f32.timesteps32_`: ins_rk_steps_f32 (chained where it chains), or with a temperature, a steady body force or the Smagorinsky closure (θ)
    ins_rk_steps_ext_f32."""
    with core.native_closure(adj.setup, θ, F32.smagorinsky_closure32):
        F32.timesteps32_(adj.cache, u, Δt, nsteps, temp=temp, θ=θ)


def _rk_adjoint_set_closure(adj, θ, θbar):
    """ins_rk_adjoint_set_closure_f32: kind 1 with θ and the device double of `θbar`, or kind 0."""
    from . import _lib
    from .operators import _thetabar_ptr

    if θ is None:
        _lib.call("ins_rk_adjoint_set_closure_f32", adj._handle, 0, 0.0, None)
    else:
        _lib.call("ins_rk_adjoint_set_closure_f32", adj._handle, 1, float(θ), _thetabar_ptr(adj.setup, θbar))


def _rk_step_pullback_(adj, ubar, tempbar, ustart, tempstart, Δt):
    """ins_rk_step_pullback_f32, with a temperature ins_rk_step_pullback_ext_f32 (the descriptor goes to the handle with every call)."""
    import ctypes as C

    from . import _lib

    setup = adj.setup
    D = setup.grid.dimension
    fp = F32._ptr(setup, _bodyforce32(setup), D) if setup.bodyforce is not None else None
    if tempbar is None:
        _lib.call("ins_rk_step_pullback_f32", adj._handle, float(1.0 / setup.Re), F32._ptr(setup, ustart, D), fp, float(Δt), F32._ptr(setup, ubar, D),
                  setup.stream)
        return
    desc = F32._temp_desc(setup)  # per call, like the forward: `setup.temperature` may have been replaced since the last one
    _lib.call("ins_rk_adjoint_set_temperature_f32", adj._handle, C.byref(desc))
    _lib.call("ins_rk_step_pullback_ext_f32", adj._handle, float(1.0 / setup.Re), F32._ptr(setup, ustart, D), F32._ptr(setup, tempstart, 0), fp, float(Δt),
              F32._ptr(setup, ubar, D), F32._ptr(setup, tempbar, 0), setup.stream)


# The Float32 precision table of the shared autograd layer (_autodiff_core.py): `f32.py` under the table's calling conventions.  The boundary
# data is constant, so `t` does not enter; any dtype but float32 raises; the steady body force is added outside the Functions, from a cached cast.
_OPS = SimpleNamespace(
    name="ad32", dtype=torch.float32,
    scalarfield=F32.scalarfield32, vectorfield=F32.vectorfield32, nfield=F32.nfield32, tensorfield=F32.tensorfield32, tb_sizes=F32._tb_sizes,
    check_dtype=_check_dtype, check_closure_inputs=_check_vec,
    bodyforce=lambda setup: None if setup.bodyforce is None else _bodyforce32(setup),
    apply_bc_u_=lambda u, t, setup, dudt: F32.apply_bc_u32_(u, setup, dudt=dudt),
    apply_bc_p_=lambda p, t, setup: F32.apply_bc_p32_(p, setup),
    apply_bc_temp_=lambda temp, t, setup: F32.apply_bc_temp32_(temp, setup),
    momentum_=lambda F, u, temp, t, setup: F32.momentum32_(F, u, setup, temp=temp),
    gravity_=F32.gravity32_, convection_diffusion_temp_=F32.convection_diffusion_temp32_, dissipation_=F32.dissipation32_,
    project_=F32.project32_, divoftensor_=F32.divoftensor32_, tensorinvariants_=F32.tensorinvariants32_,
    tensorclosure_stress_=F32.tensorclosure_stress32_,
    apply_bc_u_pullback_=F32.apply_bc_u_pullback32_, apply_bc_p_pullback_=F32.apply_bc_p_pullback32_,
    apply_bc_temp_pullback_=F32.apply_bc_temp_pullback32_, momentum_pullback_=F32.momentum_pullback32_, gravity_adjoint_=F32.gravity_adjoint32_,
    convection_diffusion_temp_adjoint_=F32.convection_diffusion_temp_adjoint32_, dissipation_adjoint_=F32.dissipation_adjoint32_,
    temperature_pullback_=F32.temperature_pullback32_, project_pullback_=F32.project_pullback32_,
    divoftensor_adjoint_=F32.divoftensor_adjoint32_, tensorclosure_pullback_=F32.tensorclosure_pullback32_,
    smagorinsky_force_=lambda s, u, θ, setup: F32.smagorinsky_force32_(
        s, u, θ, setup, F32.tensorfield32(setup) if F32._lib.load().ins_smagorinsky_force_needs_sigma(setup.handle) else None),
    smagorinsky_force_pullback_=lambda ubar, θbar, sbar, u, θ, setup: F32.smagorinsky_force_pullback32_(ubar, θbar, sbar, u, θ, setup),
    rk_adjoint_set_closure=_rk_adjoint_set_closure,
    rk_cache=_rk_cache, rk_adjoint_create=_rk_adjoint_create, rk_adjoint_destroy=_rk_adjoint_destroy, rk_steps_=_rk_steps_,
    rk_step_pullback_=_rk_step_pullback_, rk_copy_=lambda dst, src, setup, vector: dst.copy_(src),
)

# the stage Function under its Float32 spelling (`t` does not enter), as the tests call it
_StageRightHandSide = SimpleNamespace(apply=lambda u, temp, setup: core._StageRightHandSide.apply(u, temp, 0.0, setup, _OPS))


def _step_adjoint(erk, setup, psolver):
    """The reverse step's handle of (solver, tableau), as `ad._step_adjoint`."""
    return core._step_adjoint(_OPS, erk, setup, psolver)


def apply_bc_u(u, t, setup):
    """boundary_conditions.jl:114-167 with T = Float32 and constant boundary data (`t` does not enter); pullback: apply_bc_u_pullback32_."""
    _check_setup(setup, "apply_bc_u")
    return core._ApplyBCU.apply(u, t, setup, False, _OPS)


def momentum(u, temp, t, setup):
    """operators.jl:940-976 with T = Float32: convection + diffusion (momentum32_; the pullback is one launch) + a steady body force, which
    is additive and drops out of the pullback.  With a temperature field (and a temperature equation in `setup`) the gravity term is added
    (operators.jl:974), differentiable in `u` and in `temp`."""
    if temp is not None and setup.temperature is None:
        raise NotImplementedError("ad32.momentum: a temperature field needs setup.temperature (temperature_equation)")
    _check_setup(setup, "momentum")
    return core.momentum(_OPS, u, temp, t, setup)


# ------------------------------------------------------------------------------------ temperature equation
def apply_bc_temp(temp, t, setup):
    """boundary_conditions.jl:236-246 with T = Float32 and constant boundary data (`t` does not enter); pullback: apply_bc_temp_pullback32_."""
    _check_temperature(setup, "apply_bc_temp")
    return core._ApplyBCTemp.apply(temp, t, setup, _OPS)


def gravity(temp, setup):
    """operators.jl:884-931 with T = Float32; pullback: gravity_adjoint32_."""
    _check_temperature(setup, "gravity")
    return core._Gravity.apply(temp, setup, _OPS)


def convection_diffusion_temp(u, temp, setup):
    """operators.jl:692-737 with T = Float32, differentiable in `u` and in `temp`; pullback: convection_diffusion_temp_adjoint32_."""
    _check_temperature(setup, "convection_diffusion_temp")
    return core._ConvectionDiffusionTemp.apply(u, temp, setup, _OPS)


def dissipation(u, setup):
    """operators.jl:770-814 with T = Float32; the pullback (dissipation_adjoint32_) recomputes diffusion(u) in the kernel."""
    _check_temperature(setup, "dissipation")
    return core._Dissipation.apply(u, setup, _OPS)


def project(u, setup, psolver):
    """pressure.jl:52-82 with T = Float32 (project32_); pullback: project_pullback32_, the transpose for this kind of solver."""
    _check_setup(setup, "project")
    _check_psolver(setup, psolver, "project")
    return core._Project.apply(u, setup, psolver, _OPS)


# ------------------------------------------------------------------------------------ DNS-to-LES filters
# `v = Φ(u, setup_les, comp)` (lib/NeuralClosure filter.jl) on float32 fields with the exact transpose as backward (csrc/ins_filter32.hip):
# the Float32 twin of `ad.FaceAverage` / `ad.VolumeAverage`.  `Filter.apply(u, setup_les, comp, setup_dns=None)`.
FaceAverage = core.filter_function("FaceAverage", _OPS, "filter.jl:26-46")
VolumeAverage = core.filter_function("VolumeAverage", _OPS, "filter.jl:82-116")


# ------------------------------------------------------------------------------------ tensor-basis closure
def apply_bc_p(p, t, setup):
    """boundary_conditions.jl:114-206 with T = Float32 (`t` does not enter); pullback: apply_bc_p_pullback32_."""
    _check_slab(setup, "apply_bc_p")
    if tuple(p.shape) != tuple(setup.grid.N):
        raise ValueError(f"expected a field of shape {tuple(setup.grid.N)}, got {tuple(p.shape)}")
    return core._ApplyBCP.apply(p, t, setup, _OPS)


def apply_bc_p_fields(σ, t, setup):
    """`apply_bc_p` on every channel of an N + (n,) field (the stress tensor's ghost fill, operators.jl:1296)."""
    if σ.dim() != setup.grid.dimension + 1:
        raise ValueError(f"expected a field of shape {tuple(setup.grid.N)} + (n,), got {tuple(σ.shape)}")
    return core.apply_bc_p_fields(apply_bc_p, σ, t, setup)


def tensorinvariants(u, setup):
    """The invariants V of the tensor basis (N + (nv,), written on Ip) with T = Float32, without forming B."""
    _check_slab(setup, "tensorinvariants")
    return core._TensorInvariants.apply(u, setup, _OPS)


def tensorclosure_stress(u, a, setup):
    """τ = Σ_i a_i B_i(u) as a symmetric `tensorfield32` (written on Ip) in one kernel that keeps the basis in registers; the backward gives
    ubar and abar_i = <τbar, B_i>.  `a` is N + (nb,)."""
    _check_slab(setup, "tensorclosure_stress")
    return core._TensorClosureStress.apply(u, a, setup, _OPS)


def divoftensor(σ, setup):
    """operators.jl:1155-1184 with T = Float32 (pullback: divoftensor_adjoint32_) on a symmetric `tensorfield32` N + (D(D+1)/2,)."""
    _check_slab(setup, "divoftensor")
    return core._DivOfTensor.apply(σ, setup, _OPS)


lastdimcontract = core.lastdimcontract  # tensorbasis.jl:97-157


def smagorinsky_closure(setup):
    """Differentiable Smagorinsky closure `m(u, θ)` with T = Float32 (operators.jl:1284-1300), θ a 0-dim tensor: the member
    a_2 = 2 θ² d² sqrt(2 V_1), every other a_i = 0, of the tensor-basis family, as `ad.smagorinsky_closure`; gridsize² d² is held in float32."""
    _check_slab(setup, "smagorinsky_closure")
    return core.smagorinsky_closure(_OPS, setup)


def smagorinsky_force(u, θ, setup):
    """The Smagorinsky closure force of a ghost-filled float32 `u` as ONE native call (ins_smagorinsky_force_f32), with the fused pullback as backward
    (ins_smagorinsky_force_pullback_f32): `ad.smagorinsky_force` with T = Float32.  θbar is summed in double and returned in θ's dtype."""
    _check_slab(setup, "smagorinsky_force")
    return core.smagorinsky_force(_OPS, u, θ, setup)


def timestep(method, stepper, Δt, θ=None):
    """step_explicit_runge_kutta.jl:61-120 with T = Float32: one explicit Runge-Kutta step without mutation, differentiable in `stepper.u`,
    in `stepper.temp` (with the temperature equation) and (through a torch closure model `m(u, θ)`) in θ; `ad.timestep` on the Float32
    operators, stage combinations in torch arithmetic.  With a temperature field the right-hand side of a stage, (u, temp) -> (F, Ftemp), is
    one Function whose backward is two launches."""
    setup = stepper.setup
    if stepper.temp is not None and setup.temperature is None:
        raise NotImplementedError("ad32.timestep: a temperature field needs setup.temperature (temperature_equation)")
    _check_setup(setup, "timestep")
    _check_psolver(setup, stepper.psolver, "timestep")
    return core.timestep(_OPS, method, stepper, Δt, θ)


def timesteps(method, stepper, Δt, nsteps, *, θ=None, checkpoint_every=None):
    """`nsteps` calls of `ad32.timestep(method, ·, Δt)` as one Function with T = Float32: `ad.timesteps` on float32 fields, differentiable in
    `stepper.u`, with the temperature equation in `stepper.temp`, and with the Smagorinsky closure in its constant θ.

    With `setup.closure_model` the library's Smagorinsky closure of this setup (`f32.smagorinsky_closure32(setup)` or
    `ad32.smagorinsky_closure(setup)`) and `θ` its constant (a Python scalar, or a 0-dim tensor that may require grad) the closure runs inside both
    native loops (`timesteps32_(…, θ=float(θ))`; ins_smagorinsky_force_f32 and ins_smagorinsky_force_pullback_f32 in the reverse step), and ∂L/∂θ
    of all steps and chunks is summed in one device double.

    The forward is `f32.timesteps32_` (ins_rk_steps_f32; with a temperature or a steady body force ins_rk_steps_ext_f32) in chunks of
    `checkpoint_every` steps (default ceil(sqrt(nsteps))), only the chunk-start states are kept, and the backward recomputes a chunk and calls the
    native reverse step once per step (ins_rk_step_pullback_f32, with a temperature ins_rk_step_pullback_ext_f32), all in float.

    Scope: what `ad32.timestep` takes without a closure: ExplicitRungeKuttaMethod or LMWray3, 2-D / 3-D, any boundary conditions with constant
    data, a Float32 solver, no body force or a steady one, with or without `setup.temperature`.  Any other closure model, a Smagorinsky closure
    without θ, θ without a closure, callable boundary data, an unsteady body force and slab setups raise NotImplementedError: use `ad32.timestep`
    step by step (or `ins_amd.ad`)."""
    nsteps, every = core.checkpoint_interval(_OPS, nsteps, checkpoint_every)
    setup, psolver, u, temp = stepper.setup, stepper.psolver, stepper.u, stepper.temp
    core.check_rollout(_OPS, stepper, θ)
    _check_psolver(setup, psolver, "timesteps")
    if getattr(psolver, "psolver64", None) is not None and _periodic_uniform(setup):
        # measured on the 7 x 7 periodic box with a wrapped direct solver, 5 RK44 steps: timesteps32_ is 2.0e-3 from fp64, ad32.timestep 1.0e-7
        raise NotImplementedError("ad32.timesteps: on an all-periodic uniform box the native Float32 loop (timesteps32_) does not refill the ghost "
                                  "volumes between a wrapped solver's projections, so its rollout is not the step ad32.timestep differentiates; "
                                  "use f32.psolver_spectral32, or ad32.timestep step by step")
    _check_vec(setup, u)
    if temp is not None and tuple(temp.shape) != tuple(setup.grid.N):
        raise ValueError(f"expected a temperature field of shape {tuple(setup.grid.N)}, got {tuple(temp.shape)}")
    return core.timesteps(_OPS, method, stepper, Δt, nsteps, every, θ=θ)
