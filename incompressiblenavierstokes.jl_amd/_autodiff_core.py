"""The autograd layer that `ins_amd.ad` (autodiff.py, fp64) and `ins_amd.ad32` (autodiff32.py, Float32) share: the layout and save-for-backward
helpers, the `torch.autograd.Function`s over the in-place forwards and their pullbacks, the differentiable Smagorinsky closure and the Runge-Kutta
stage loop of `timestep`, each written once against a precision table `ops`.

A public module builds one table and passes it as the last, non-tensor argument of every Function (`_Momentum.apply(u, t, setup, ops)`).  The table
gives every native call ONE calling convention; what `operators.py` and `f32.py` spell differently (a time argument the Float32 family does not take,
the literal 0.0 time of the fp64 pullbacks, `momentum32_(F, u, setup, temp=)`) is absorbed by the table's adapters, and where the two modules differ
in policy (dtype strictness, where the body force is added) the table carries a hook.  The refusals of the public entry points stay in the public
modules.  Nothing here touches the native library except through the table, so a table of plain torch maps drives all of it without a device
(tests/test_autodiff_core_cpu.py).
"""
from types import SimpleNamespace

import numpy as np
import torch

from ._step_route import Closure, Force, classify, mark_ad_closure, mark_library_closure, smagorinsky_of
from .setup import _fortran_strides
from .time_steppers import LMWray3, _lmwray3_as_erk, create_stepper

# The precision table `ops` is a namespace of
#   name, dtype                 "ad" / "ad32" for messages, the torch dtype of the fields
#   allocators of zero fields   scalarfield(setup), vectorfield(setup), nfield(setup, ncomp), tensorfield(setup); tb_sizes(setup) -> (nb, nv, ns)
#   policy hooks                check_dtype(x): ad32 raises TypeError for a tensor that is not float32, ad converts silently
#                               check_closure_inputs(setup, u or None, *others): what the tensor-basis Functions refuse before converting anything
#                               bodyforce(setup): the field added to F outside the Functions, or None (fp64 adds it inside `momentum_`)
#   in-place forwards           apply_bc_u_(u, t, setup, dudt), apply_bc_p_(p, t, setup), apply_bc_temp_(temp, t, setup),
#                               momentum_(F, u, temp or None, t, setup), gravity_(F, temp, setup), convection_diffusion_temp_(c, u, temp, setup),
#                               dissipation_(diss, diff, u, setup), project_(u, setup, psolver, p), divoftensor_(s, σ, setup),
#                               tensorinvariants_(V, u, setup), tensorclosure_stress_(τ, u, a, setup)
#   pullbacks                   apply_bc_u_pullback_(φbar, setup), apply_bc_p_pullback_(φbar, setup), apply_bc_temp_pullback_(tempbar, setup),
#                               momentum_pullback_(ubar, φbar, u, setup), gravity_adjoint_(tempbar, φbar, setup),
#                               convection_diffusion_temp_adjoint_(ubar or None, tempbar or None, cbar, u, temp, setup),
#                               dissipation_adjoint_(ubar, cbar, u, setup), temperature_pullback_(ubar, tempbar, Fbar, cbar, u, temp, setup),
#                               project_pullback_(φbar, setup, psolver, pwork), divoftensor_adjoint_(σbar, sbar, setup),
#                               tensorclosure_pullback_(ubar, abar, τbar, Vbar, u, a, setup)
#   Smagorinsky closure force   smagorinsky_force_(s, u, θ, setup): the one-call native force, θ a Python float;
#                               smagorinsky_force_pullback_(ubar, θbar, sbar, u, θ, setup): ubar overwritten, θbar (a 0-dim float64 tensor on the
#                               setup's device, or None) added to
# Every call works in place on its first argument(s) and returns what it wrote.


# ------------------------------------------------------------------------------------ layout and save-for-backward
def _field(ops, setup, x, vector):
    """`x` itself when it already has the library's field layout, else a copy in that layout (cotangents from torch are often expanded
    views with zero strides, or permuted the other way).  `vector` as in `Setup.ptr`: False (scalar field), True (D components) or an int
    (an N + (n,) field; only there another shape raises ValueError)."""
    ops.check_dtype(x)
    g = setup.grid
    shape = tuple(g.N) + ((g.dimension,) if vector is True else (vector,) if vector is not False else ())
    if vector is not True and vector is not False and tuple(x.shape) != shape:
        raise ValueError(f"expected a field of shape {shape}, got {tuple(x.shape)}")
    if x.dtype == ops.dtype and x.device == setup.device and tuple(x.shape) == shape and tuple(x.stride()) == _fortran_strides(shape):
        return x
    return _copy(ops, setup, x, vector)


def _copy(ops, setup, x, vector):
    """A fresh field (library layout) holding `x`: the in-place forwards and pullbacks work on it."""
    ops.check_dtype(x)
    f = ops.vectorfield(setup) if vector is True else ops.scalarfield(setup) if vector is False else ops.nfield(setup, vector)
    f.copy_(x.detach())
    return f


def _save_inputs(ops, ctx, setup, items):
    """The fields a backward reads, `items` = (tensor, vector) pairs: an input that already is a library field goes through
    save_for_backward, so an in-place change of it before backward() raises instead of giving a wrong gradient; a layout copy is private
    to the Function."""
    fields, saved, copies = [], [], []
    for x, vector in items:
        f = _field(ops, setup, x, vector)
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


# ------------------------------------------------------------------------------------ ghost fill
class _ApplyBCU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, t, setup, dudt, ops):
        ctx.setup, ctx.ops = setup, ops
        return ops.apply_bc_u_(_copy(ops, setup, u, True), t, setup, dudt)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.apply_bc_u_pullback_(_copy(ops, s, g, True), s), None, None, None, None


class _ApplyBCP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        return ops.apply_bc_p_(_copy(ops, setup, p, False), t, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.apply_bc_p_pullback_(_copy(ops, s, g, False), s), None, None, None


class _ApplyBCTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, t, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        return ops.apply_bc_temp_(_copy(ops, setup, temp, False), t, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.apply_bc_temp_pullback_(_copy(ops, s, g, False), s), None, None, None


# ------------------------------------------------------------------------------------ momentum and the temperature equation
class _Momentum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, t, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        (uf,) = _save_inputs(ops, ctx, setup, [(u, True)])
        return ops.momentum_(ops.vectorfield(setup), uf, None, t, setup)

    @staticmethod
    def backward(ctx, g):  # the body force is additive: it drops out
        s, ops = ctx.setup, ctx.ops
        (u,) = _saved_inputs(ctx)
        return ops.momentum_pullback_(ops.vectorfield(s), _field(ops, s, g, True), u, s), None, None, None


class _Gravity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, temp, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        return ops.gravity_(ops.vectorfield(setup), _field(ops, setup, temp, False), setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.gravity_adjoint_(ops.scalarfield(s), _field(ops, s, g, True), s), None, None


class _ConvectionDiffusionTemp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, temp, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        uf, tf = _save_inputs(ops, ctx, setup, [(u, True), (temp, False)])
        return ops.convection_diffusion_temp_(ops.scalarfield(setup), uf, tf, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        u, temp = _saved_inputs(ctx)
        ubar = ops.vectorfield(s) if ctx.needs_input_grad[0] else None
        tempbar = ops.scalarfield(s) if ctx.needs_input_grad[1] else None
        if ubar is not None or tempbar is not None:
            ops.convection_diffusion_temp_adjoint_(ubar, tempbar, _field(ops, s, g, False), u, temp, s)
        return ubar, tempbar, None, None


class _Dissipation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        (uf,) = _save_inputs(ops, ctx, setup, [(u, True)])
        return ops.dissipation_(ops.scalarfield(setup), ops.vectorfield(setup), uf, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        (u,) = _saved_inputs(ctx)
        return ops.dissipation_adjoint_(ops.vectorfield(s), _field(ops, s, g, False), u, s), None, None


class _StageRightHandSide(torch.autograd.Function):
    """(u, temp) -> (F, Ftemp) of one Runge-Kutta stage (step_explicit_runge_kutta.jl:79-83): F = momentum(u, temp) (in Float32 without the
    body force, which `timestep` adds outside), Ftemp = convection_diffusion_temp(u, temp) + dissipation(u).  The backward is two launches:
    momentum_pullback_, then temperature_pullback_."""

    @staticmethod
    def forward(ctx, u, temp, t, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        ctx.set_materialize_grads(False)
        uf, tf = _save_inputs(ops, ctx, setup, [(u, True), (temp, False)])
        F = ops.momentum_(ops.vectorfield(setup), uf, tf, t, setup)
        Ftemp = ops.convection_diffusion_temp_(ops.scalarfield(setup), uf, tf, setup)
        if setup.temperature.dodissipation:
            ops.dissipation_(Ftemp, ops.vectorfield(setup), uf, setup)
        return F, Ftemp

    @staticmethod
    def backward(ctx, gF, gT):
        s, ops = ctx.setup, ctx.ops
        if gF is None and gT is None:
            return None, None, None, None, None
        u, temp = _saved_inputs(ctx)
        Fbar = ops.vectorfield(s) if gF is None else _field(ops, s, gF, True)
        cbar = ops.scalarfield(s) if gT is None else _field(ops, s, gT, False)
        ubar = ops.momentum_pullback_(ops.vectorfield(s), Fbar, u, s)
        ubar, tempbar = ops.temperature_pullback_(ubar, ops.scalarfield(s), Fbar, cbar, u, temp, s)
        return ubar, tempbar, None, None, None


def momentum(ops, u, temp, t, setup):
    """F = momentum(u) [+ gravity(temp)] [+ the body force, where the precision adds it outside the Function], in this order."""
    F = _Momentum.apply(u, t, setup, ops)
    if temp is not None:
        F = F + _Gravity.apply(temp, setup, ops)
    f = ops.bodyforce(setup)
    return F if f is None else F + f


# ------------------------------------------------------------------------------------ projection
class _Project(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, psolver, ops):
        ctx.setup, ctx.psolver, ctx.ops = setup, psolver, ops
        return ops.project_(_copy(ops, setup, u, True), setup, psolver, ops.scalarfield(setup))

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.project_pullback_(_copy(ops, s, g, True), s, ctx.psolver, ops.scalarfield(s)), None, None, None


# ------------------------------------------------------------------------------------ DNS-to-LES filters
class _Filter(torch.autograd.Function):
    """`v = Φ(u, setup_les, comp)` (lib/NeuralClosure filter.jl) with the exact transpose as backward (csrc/ins_filter.hip, csrc/ins_filter32.hip):
    a loss on filtered quantities of a differentiable DNS step.  `kind` names the filter in `neuralclosure`, which dispatches on the dtype itself."""

    @staticmethod
    def forward(ctx, u, setup_les, comp, setup_dns, kind, ops):
        from . import neuralclosure as nc

        dns = setup_dns or nc.dns_setup_of(setup_les, int(comp))
        ctx.les, ctx.dns, ctx.comp, ctx.filter, ctx.ops = setup_les, dns, int(comp), getattr(nc, kind)(), ops
        return ctx.filter(_field(ops, dns, u, True), setup_les, int(comp), setup_dns=dns)

    @staticmethod
    def backward(ctx, g):
        ops = ctx.ops
        ubar = ctx.filter.pullback_(ops.vectorfield(ctx.dns), _field(ops, ctx.les, g, True), ctx.les, ctx.comp, ctx.dns)
        return ubar, None, None, None, None, None


def filter_function(kind, ops, doc):
    """`FaceAverage` / `VolumeAverage` of one precision: `.apply(u, setup_les, comp, setup_dns=None)`."""
    return SimpleNamespace(apply=lambda u, setup_les, comp, setup_dns=None: _Filter.apply(u, setup_les, comp, setup_dns, kind, ops), __doc__=doc)


# ------------------------------------------------------------------------------------ tensor-basis closure
class _DivOfTensor(torch.autograd.Function):
    @staticmethod
    def forward(ctx, σ, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        ops.check_closure_inputs(setup, None, σ)
        return ops.divoftensor_(ops.vectorfield(setup), _field(ops, setup, σ, ops.tb_sizes(setup)[2]), setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        return ops.divoftensor_adjoint_(ops.tensorfield(s), _field(ops, s, g, True), s), None, None


class _TensorInvariants(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        ops.check_closure_inputs(setup, u)
        V = ops.nfield(setup, ops.tb_sizes(setup)[1])
        (uf,) = _save_inputs(ops, ctx, setup, [(u, True)])
        return ops.tensorinvariants_(V, uf, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        (u,) = _saved_inputs(ctx)
        Vbar = _field(ops, s, g, ops.tb_sizes(s)[1])
        return ops.tensorclosure_pullback_(ops.vectorfield(s), None, None, Vbar, u, None, s), None, None


class _TensorClosureStress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, a, setup, ops):
        ctx.setup, ctx.ops = setup, ops
        ops.check_closure_inputs(setup, u, a)
        uf, af = _save_inputs(ops, ctx, setup, [(u, True), (a, ops.tb_sizes(setup)[0])])
        return ops.tensorclosure_stress_(ops.tensorfield(setup), uf, af, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        u, a = _saved_inputs(ctx)
        nb, _, ns = ops.tb_sizes(s)
        abar = ops.nfield(s, nb)
        ubar = ops.tensorclosure_pullback_(ops.vectorfield(s), abar, _field(ops, s, g, ns), None, u, a, s)
        return ubar, abar, None, None


def lastdimcontract(a, b):
    """tensorbasis.jl:97-157: c[I] = Σ_i a[I, i] b[I, i, ...] — plain torch (its pullback is torch's)."""
    return (a.reshape(a.shape + (1,) * (b.dim() - a.dim())) * b).sum(dim=a.dim() - 1)


def apply_bc_p_fields(apply_bc_p, σ, t, setup):
    """`apply_bc_p(p, t, setup)` on every channel of an N + (n,) field (the stress tensor's ghost fill, operators.jl:1296)."""
    return torch.stack([apply_bc_p(σ[..., q], t, setup) for q in range(σ.shape[-1])], dim=-1)


def _gridsize2(setup):
    """gridsize² = Σ_α Δ_α[I_α]² over the padded array (operators.jl:1137), in float64."""
    g = setup.grid
    D = g.dimension
    d2 = torch.zeros(tuple(g.N), dtype=torch.float64, device=setup.device)
    for α in range(D):
        shape = [1] * D
        shape[α] = g.N[α]
        d2 = d2 + torch.as_tensor(np.asarray(g.Δ[α], dtype=np.float64) ** 2, device=setup.device).reshape(shape)
    return d2


def smagorinsky_closure(ops, setup):
    """The differentiable Smagorinsky closure `m(u, θ)` (operators.jl:1284-1300): the member a_2 = 2 θ² d² sqrt(2 V_1), every other a_i = 0, of
    the tensor-basis family.  gridsize² d² is summed in float64, cut to Ip, and held in the precision's dtype."""
    g = setup.grid
    D = g.dimension
    nb = ops.tb_sizes(setup)[0]
    ip = tuple(slice(lo, hi) for lo, hi in g.Ip)
    pads = [q for α in reversed(range(D)) for q in (g.Ip[α][0], g.N[α] - g.Ip[α][1])]
    d2 = _gridsize2(setup)[ip].to(ops.dtype)

    def closure(u, θ):
        θ = torch.as_tensor(θ, dtype=ops.dtype, device=setup.device)
        V = _TensorInvariants.apply(u, setup, ops)
        # Ip only: sqrt has no derivative at the zeros outside.  Inside, where S:S = 0 the contribution is defined as zero: sqrt is taken of 1 there and
        # the result masked, so its backward is 0 instead of 0 / 0 (the forward value, 0, and everything where S:S > 0 are unchanged)
        V1 = V[ip + (0,)]
        live = V1 > 0
        mag = torch.where(live, torch.sqrt(2 * torch.where(live, V1, torch.ones_like(V1))), torch.zeros_like(V1))
        a2 = torch.nn.functional.pad(2 * θ * θ * d2 * mag, pads)
        z = torch.zeros_like(a2)
        a = torch.stack([z, a2] + [z] * (nb - 2), dim=-1)
        τ = apply_bc_p_fields(lambda p, t, s: _ApplyBCP.apply(p, t, s, ops), _TensorClosureStress.apply(u, a, setup, ops), 0.0, setup)
        return _DivOfTensor.apply(τ, setup, ops)

    return mark_ad_closure(closure, ops.name, setup)  # `timesteps` takes it for the closure of its native loops (the step functions do not route on it)


class _SmagorinskyForce(torch.autograd.Function):
    """s = m(u, θ), the Smagorinsky closure force of the ghost-filled `u` (operators.jl:1284-1300) as the one native call, θ a 0-dim tensor.  The
    backward is the fused pullback (csrc/ins_smagpullback_kernels.h): ubar, and θbar = 2θ <σ̄, σ̂> from the same pass."""

    @staticmethod
    def forward(ctx, u, θ, setup, ops):
        ctx.setup, ctx.ops, ctx.θ = setup, ops, float(θ)
        ops.check_closure_inputs(setup, u)
        (uf,) = _save_inputs(ops, ctx, setup, [(u, True)])
        return ops.smagorinsky_force_(ops.vectorfield(setup), uf, ctx.θ, setup)

    @staticmethod
    def backward(ctx, g):
        s, ops = ctx.setup, ctx.ops
        (u,) = _saved_inputs(ctx)
        θbar = torch.zeros((), dtype=torch.float64, device=s.device) if ctx.needs_input_grad[1] else None
        ubar, θbar = ops.smagorinsky_force_pullback_(ops.vectorfield(s), θbar, _field(ops, s, g, True), u, ctx.θ, s)
        return ubar, θbar, None, None


def smagorinsky_force(ops, u, θ, setup):
    """`_SmagorinskyForce` with θ a Python scalar or a 0-dim tensor; θbar comes back in θ's dtype and on its device."""
    θ = θ if isinstance(θ, torch.Tensor) else torch.tensor(float(θ), dtype=ops.dtype)
    if θ.dim() != 0:
        raise ValueError(f"{ops.name}.smagorinsky_force: θ must be a scalar or a 0-dim tensor")
    return _SmagorinskyForce.apply(u, θ, setup, ops)


class native_closure:
    """While a rollout's native forward runs: `setup.closure_model` carries the tags on which `timesteps_` / `timesteps32_` put the Smagorinsky
    closure into the native stage loop.  The fused closure has them; the differentiable one is replaced, for the duration, by a stand-in made by
    `make(setup)` on first use and kept on the setup."""

    def __init__(self, setup, θ, make):
        self.setup, self.on, self.make = setup, θ is not None and classify(setup).closure is not Closure.LIBRARY, make

    def __enter__(self):
        if self.on:
            s = self.setup
            self.saved = s.closure_model
            if getattr(s, "_ad_native_closure", None) is None:
                real = []

                def closure(u, θ):  # only a host-driven stage loop evaluates it
                    if not real:
                        real.append(self.make(s))
                    return real[0](u, θ)

                s._ad_native_closure = mark_library_closure(closure, s)
            s.closure_model = s._ad_native_closure

    def __exit__(self, *exc):
        if self.on:
            self.setup.closure_model = self.saved
        return False


# ------------------------------------------------------------------------------------ time stepping
def timestep(ops, method, stepper, Δt, θ):
    """step_explicit_runge_kutta.jl:61-120: one explicit Runge-Kutta step without mutation (the refusals are the caller's).  The stage
    combinations are torch arithmetic; with a temperature field the right-hand side of a stage, (u, temp) -> (F, Ftemp), is one Function whose
    backward is two launches.  F is summed in the order momentum (+ gravity), body force, closure."""
    setup, psolver, u, temp, t, n = stepper.setup, stepper.psolver, stepper.u, stepper.temp, stepper.t, stepper.n
    m = setup.closure_model
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    A, c = erk.A, erk.c
    tstart, ustart, tempstart, ku, ktemp = t, u, temp, [], []
    for i in range(len(erk.b)):
        u = _ApplyBCU.apply(u, t, setup, False, ops)
        if temp is None:
            F = momentum(ops, u, None, t, setup)
        else:
            temp = _ApplyBCTemp.apply(temp, t, setup, ops)
            F, Ftemp = _StageRightHandSide.apply(u, temp, t, setup, ops)
            f = ops.bodyforce(setup)
            if f is not None:
                F = F + f
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
        u = _ApplyBCU.apply(u, t, setup, False, ops)
        u = _Project.apply(u, setup, psolver, ops)
    u = _ApplyBCU.apply(u, t, setup, False, ops)
    if temp is not None:
        temp = _ApplyBCTemp.apply(temp, t, setup, ops)
    return create_stepper(method, setup=setup, psolver=psolver, u=u, temp=temp, t=t, n=n + 1)


# ------------------------------------------------------------------------------------ member forms: B trajectories in one graph
# fp64 only (the ensemble handle is): the Functions take the `EnsembleCache` where the single-field ones take (setup, ops), and act on (B,) + N + (2,)
# tensors in the layout of `vectorfields`.  Copy and save-for-backward rules are those of `_copy`, `_field` and `_save_inputs` above.
def _ens_copy(cache, x):
    """A fresh ensemble field (the layout of `vectorfields`) holding `x`: the in-place member forwards and pullbacks work on it."""
    from .setup import vectorfields

    f = vectorfields(cache.setup, cache.B)
    if tuple(x.shape) != tuple(f.shape):
        raise ValueError(f"ensemble field must have shape {tuple(f.shape)} (use vectorfields), got {tuple(x.shape)}")
    f.copy_(x.detach())
    return f


def _ens_field(cache, x):
    """`x` itself when it already is an ensemble field of the cache (float64, on its device, every member in the library's layout, members not
    overlapping), else a copy in the layout of `vectorfields` (a cotangent with foreign strides, an expanded view)."""
    from .time_steppers import _ensemble_ustride

    try:
        _ensemble_ustride(cache, x)
        return x
    except (TypeError, ValueError):
        return _ens_copy(cache, x)


def _ens_save(ctx, cache, x):
    """The ensemble field a backward reads: an input that already is one goes through save_for_backward (an in-place edit before backward() raises), a
    layout copy is private to the Function."""
    f = _ens_field(cache, x)
    ctx.save_for_backward(*((x,) if f is x else ()))
    ctx.copy = None if f is x else f
    return f


def _ens_saved(ctx):
    return ctx.saved_tensors[0] if ctx.copy is None else ctx.copy


class _EnsembleApplyBCU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, cache):
        from .time_steppers import ensemble_apply_bc_u_

        ctx.cache = cache
        return ensemble_apply_bc_u_(cache, _ens_copy(cache, U))

    @staticmethod
    def backward(ctx, g):
        from .time_steppers import ensemble_apply_bc_u_pullback_

        return ensemble_apply_bc_u_pullback_(ctx.cache, _ens_copy(ctx.cache, g)), None


class _EnsembleMomentum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, cache):
        from .setup import vectorfields
        from .time_steppers import ensemble_momentum_

        ctx.cache = cache
        return ensemble_momentum_(cache, vectorfields(cache.setup, cache.B), _ens_save(ctx, cache, U))

    @staticmethod
    def backward(ctx, g):
        from .setup import vectorfields
        from .time_steppers import ensemble_momentum_pullback_

        c = ctx.cache
        return ensemble_momentum_pullback_(c, vectorfields(c.setup, c.B), _ens_field(c, g), _ens_saved(ctx)), None


class _EnsembleProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, cache):
        from .time_steppers import ensemble_project_

        ctx.cache = cache
        return ensemble_project_(cache, _ens_copy(cache, U))

    @staticmethod
    def backward(ctx, g):
        from .time_steppers import ensemble_project_pullback_

        return ensemble_project_pullback_(ctx.cache, _ens_copy(ctx.cache, g)), None


def timestep_ensemble(method, cache, U, Δt, θ, closure):
    """The stage loop of `timestep` on the member Functions (the refusals are the caller's): one explicit Runge-Kutta step of all B members of `U`
    without mutation.  Stage combinations are torch arithmetic on the whole (B, …) tensor, `closure(u, θ)` is called once per stage on all members, F
    is summed in the order momentum, closure.

    Ghost fills of `timestep` that are dropped here because they are the identity, in value and in the backward:
      * the fill before every projection: `_EnsembleProject` is E·P·R, it reads the interior only (through its periodic images), and its pullback
        returns zero ghost cotangents, on which the fill's transpose is the identity;
      * the fill after every projection, the one at the top of stages 2 … s and the one that ends the step: `_EnsembleProject` ends with the periodic
        extension E, fill = E·R and R·E = I, so fill·E = E and Eᵀ·fillᵀ = Eᵀ.
    Only the fill at the top of the first stage stays: the caller's `U` may come with any ghost volumes."""
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    A = erk.A
    ustart, ku = U, []
    u = _EnsembleApplyBCU.apply(U, cache)
    for i in range(len(erk.b)):
        F = _EnsembleMomentum.apply(u, cache)
        if closure is not None:
            F = F + closure(u, θ)
        ku.append(F)
        u = ustart
        for j in range(i + 1):
            if A[i, j] != 0:
                u = u + (Δt * A[i, j]) * ku[j]
        u = _EnsembleProject.apply(u, cache)
    return u


# ------------------------------------------------------------------------------------ checkpointed rollouts
# The table's part of a rollout (the only native calls of this section):
#   rk_cache(erk, setup, psolver)                           the forward's native cache (`ERKCache` / `ERKCache32`)
#   rk_adjoint_create(erk, setup, psolver) -> handle        the work arrays of the native reverse step; rk_adjoint_destroy(handle)
#   rk_steps_(adj, u, temp or None, t, Δt, nsteps[, θ])     the native multi-step loop of that setup, in place (`timesteps_` / `timesteps32_`); θ: a
#                                                           Python float, given only with the Smagorinsky closure
#   rk_adjoint_set_closure(adj, θ or None, θbar or None)    the Smagorinsky closure on the reverse step's handle (θbar: 0-dim float64 device tensor
#                                                           that every later step pullback adds to), None switches it off
#   rk_step_pullback_(adj, ubar, tempbar or None, ustart, tempstart or None, Δt)      one native reverse step, in place on (ubar, tempbar)
#   rk_copy_(dst, src, setup, vector)                       a field copy by the library's own pass
class _StepAdjoint:
    """The work arrays of the native reverse step (csrc/ins_rk_adjoint.hip: `ins_rk_adjoint_t` / `ins_rk_adjoint32_t`), with the forward's native
    cache beside it."""

    def __init__(self, ops, erk, setup, psolver):
        self.ops, self.erk, self.setup = ops, erk, setup
        self.cache = ops.rk_cache(erk, setup, psolver)
        self._handle = ops.rk_adjoint_create(erk, setup, psolver)
        self.closure_on = False

    def steps_(self, u, temp, t, Δt, nsteps, θ=None):
        """`nsteps` native steps on (u, temp), in place; θ (a Python float): with the Smagorinsky closure."""
        if θ is None:
            self.ops.rk_steps_(self, u, temp, t, Δt, nsteps)
        else:
            self.ops.rk_steps_(self, u, temp, t, Δt, nsteps, θ)
        return u, temp

    def set_closure_(self, θ, θbar=None):
        """The Smagorinsky closure with constant θ on the handle: every later `step_pullback_` carries it and adds ∂L/∂θ to `θbar`.  None clears it."""
        if θ is not None or self.closure_on:
            self.ops.rk_adjoint_set_closure(self, θ, θbar)
            self.closure_on = θ is not None

    def step_pullback_(self, ubar, ustart, Δt, tempbar=None, tempstart=None):
        """(ubar, tempbar): ∂L/∂(u_out, temp_out) -> ∂L/∂(ustart, tempstart), in place: the whole reverse sweep of one step is this one call."""
        self.ops.rk_step_pullback_(self, ubar, tempbar, ustart, tempstart, Δt)
        return ubar if tempbar is None else (ubar, tempbar)

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                self.ops.rk_adjoint_destroy(h)
            except Exception:
                pass


def _step_adjoint(ops, erk, setup, psolver):
    """One `_StepAdjoint` per (solver, tableau), kept on the solver."""
    key = (np.asarray(erk.A, dtype=np.float64).tobytes(), np.asarray(erk.c, dtype=np.float64).tobytes())
    store = psolver.__dict__.setdefault("_ad_step_adjoints", {})
    if key not in store:
        store[key] = _StepAdjoint(ops, erk, setup, psolver)
    return store[key]


class _TimeSteps(torch.autograd.Function):
    """(u, temp) -> (u, temp) after nsteps Runge-Kutta steps, `temp` possibly None; θ: None, or the 0-dim tensor of the Smagorinsky constant.  Saved:
    the state at the start of every chunk of `every` steps, nothing else.  Both field cotangents are always propagated (one native call per step
    serves both); autograd drops the one nobody asked for.  θbar is collected in one device double, zeroed once per backward, that every reverse
    step of every chunk adds to."""

    @staticmethod
    def forward(ctx, u, temp, θ, adj, ops, t, Δt, nsteps, every):
        setup = adj.setup
        out = _copy(ops, setup, u, True)
        tout = None if temp is None else _copy(ops, setup, temp, False)
        ctx.adj, ctx.ops, ctx.t, ctx.Δt, ctx.nsteps, ctx.every = adj, ops, t, Δt, nsteps, every
        ctx.θ, ctx.θlike = (None, None) if θ is None else (float(θ), (θ.dtype, θ.device))
        kw = {} if θ is None else {"θ": ctx.θ}
        ctx.checkpoints = []
        for start in range(0, nsteps, every):
            ctx.checkpoints.append((_copy(ops, setup, out, True), None if tout is None else _copy(ops, setup, tout, False)))
            adj.steps_(out, tout, t + start * Δt, Δt, min(every, nsteps - start), **kw)
        return out, tout

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, gtemp):
        adj, ops, Δt, nsteps, every = ctx.adj, ctx.ops, ctx.Δt, ctx.nsteps, ctx.every
        setup = adj.setup
        coupled = ctx.checkpoints[0][1] is not None
        ubar = _copy(ops, setup, g, True)
        tempbar = _copy(ops, setup, gtemp, False) if coupled else None
        # the step-start states of one chunk after its checkpoint
        bufs = [(ops.vectorfield(setup), ops.scalarfield(setup) if coupled else None) for _ in range(min(every, nsteps) - 1)]
        starts = list(range(0, nsteps, every))
        kw, θbar = {}, None
        if ctx.θ is not None:
            kw = {"θ": ctx.θ}
            if ctx.needs_input_grad[2]:
                θbar = torch.zeros((), dtype=torch.float64, device=setup.device)
            adj.set_closure_(ctx.θ, θbar)
        try:
            for q in reversed(range(len(starts))):
                n = min(every, nsteps - starts[q])
                states = [ctx.checkpoints[q]]
                for j in range(1, n):
                    bu, bt = bufs[j - 1]
                    ops.rk_copy_(bu, states[j - 1][0], setup, True)
                    if coupled:
                        ops.rk_copy_(bt, states[j - 1][1], setup, False)
                    adj.steps_(bu, bt, ctx.t + (starts[q] + j - 1) * Δt, Δt, 1, **kw)
                    states.append((bu, bt))
                for j in reversed(range(n)):
                    adj.step_pullback_(ubar, states[j][0], Δt, tempbar, states[j][1])
                ctx.checkpoints[q] = None
        finally:
            if ctx.θ is not None:
                adj.set_closure_(None)
        if θbar is not None:
            θbar = θbar.to(dtype=ctx.θlike[0], device=ctx.θlike[1])
        return ubar, tempbar, θbar, None, None, None, None, None, None


# module, dtype name and pressure solvers of the two precision tables, for the messages that send a caller to the other one
_PRECISIONS = {torch.float64: ("ad", "float64", "default_psolver and its kin"), torch.float32: ("ad32", "float32", "f32.default_psolver32 / f32.psolver_wrap32")}


def check_rollout(ops, stepper, θ):
    """What `ad.timesteps` and `ad32.timesteps` refuse alike.  The first check that applies names the reason, in this order:
      TypeError            `u` of another dtype; `temp` of another dtype than `u`; a pressure solver of the other precision
      ValueError           a temperature field without a temperature equation
      NotImplementedError  a closure model other than the library's Smagorinsky closure of this setup with its θ (or θ without one); a temperature
                           equation without a field; a slab side; callable velocity data; callable temperature data; an unsteady body force
    What one precision adds comes after this list, the shape ValueErrors of the fields last.  The setup is classified (`_step_route.classify`) once
    the types are right: a stepper of the wrong precision is turned away whatever its setup is."""
    from . import f32

    setup, psolver, u, temp = stepper.setup, stepper.psolver, stepper.u, stepper.temp
    (name, dt, solvers), (other, odt, osolvers) = _PRECISIONS[ops.dtype], _PRECISIONS[torch.float32 if ops.dtype == torch.float64 else torch.float64]
    if u.dtype != ops.dtype:
        raise TypeError(f"{name}.timesteps: fields must be {dt} torch tensors ({odt} fields: {other}.timesteps)")
    if temp is not None and temp.dtype != ops.dtype:
        raise TypeError(f"{name}.timesteps: a {dt} u with a {odt} temp: give both fields in one precision")
    if isinstance(psolver, f32.psolver_spectral32) != (ops.dtype == torch.float32):
        raise TypeError(f"{name}.timesteps: a {dt} u with a {odt} psolver ({dt} fields: {solvers}; {odt} fields: {other}.timesteps with {osolvers})")
    if temp is not None and setup.temperature is None:
        raise ValueError("a temperature field needs setup.temperature (temperature_equation)")
    facts = classify(setup, temp, θ)
    stepwise = f"use {name}.timestep step by step"
    if (facts.closure is not Closure.NONE or θ is not None) and not (θ is not None and smagorinsky_of(facts, name, ops.dtype)):
        raise NotImplementedError(f"{name}.timesteps: a closure model is not part of the native reverse loop; {stepwise}")
    if temp is None and setup.temperature is not None:
        raise NotImplementedError(f"{name}.timesteps: a setup with a temperature equation takes stepper.temp in the native reverse loop; without one "
                                  f"{stepwise}")
    # the rest the Float32 family does not run at all: its step-by-step route is the fp64 one
    if facts.slab:
        raise NotImplementedError(f"{name}.timesteps: slab (halo) setups are not supported; use ad.timestep step by step")
    if facts.bc_u_callable:
        raise NotImplementedError(f"{name}.timesteps: callable Dirichlet data needs the host between the stages; use ad.timestep step by step")
    if temp is not None and facts.bc_temp_callable:
        raise NotImplementedError(f"{name}.timesteps: callable Dirichlet data of the temperature needs the host between the stages; use ad.timestep step "
                                  "by step")
    if facts.force is Force.UNSTEADY:
        raise NotImplementedError(f"{name}.timesteps: an unsteady body force is evaluated in fp64 on the host; use ad.timestep step by step")


def checkpoint_interval(ops, nsteps, checkpoint_every):
    """(nsteps, every) of a rollout: ceil(sqrt(nsteps)) steps per chunk unless told otherwise."""
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError(f"{ops.name}.timesteps: nsteps must be >= 1, got {nsteps}")
    every = int(np.ceil(np.sqrt(nsteps))) if checkpoint_every is None else int(checkpoint_every)
    if every < 1:
        raise ValueError(f"{ops.name}.timesteps: checkpoint_every must be >= 1, got {checkpoint_every}")
    return nsteps, min(every, nsteps)


def timesteps(ops, method, stepper, Δt, nsteps, every, adj=None, θ=None):
    """`nsteps` Runge-Kutta steps as one Function (the refusals are the caller's): the native multi-step loop forward in chunks of `every` steps,
    the state at every chunk start kept, one native reverse step per step backward.  `adj`: the reverse step's handle, by default the one kept
    on the solver.  θ: None, or the constant of the setup's Smagorinsky closure (a Python scalar, or a 0-dim tensor that may require grad)."""
    setup, psolver, u, temp = stepper.setup, stepper.psolver, stepper.u, stepper.temp
    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    if adj is None:
        adj = _step_adjoint(ops, erk, setup, psolver)
    t = float(stepper.t)
    if θ is not None:
        θ = θ if isinstance(θ, torch.Tensor) else torch.tensor(float(θ), dtype=ops.dtype)
        if θ.dim() != 0:
            raise ValueError(f"{ops.name}.timesteps: θ must be a scalar or a 0-dim tensor")
    if torch.is_grad_enabled() and (u.requires_grad or (temp is not None and temp.requires_grad) or (θ is not None and θ.requires_grad)):
        out, tout = _TimeSteps.apply(u, temp, θ, adj, ops, t, float(Δt), nsteps, every)
    else:  # nothing to save: one native call
        kw = {} if θ is None else {"θ": float(θ)}
        out, tout = adj.steps_(_copy(ops, setup, u, True), None if temp is None else _copy(ops, setup, temp, False), t, float(Δt), nsteps, **kw)
    return create_stepper(method, setup=setup, psolver=psolver, u=out, temp=tout, t=t + nsteps * erk.c[-1] * Δt, n=stepper.n + nsteps)
