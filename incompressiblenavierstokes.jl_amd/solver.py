"""`solve_unsteady` and the CFL time step (solver.jl)."""
import ctypes as C
import math
import os

import torch

from . import _lib
from .pressure import default_psolver
from .setup import copyfield, vectorfields
from .time_steppers import (LMWray3, RKMethods, _ensemble_ustride, create_stepper, get_cfl_timestep_ensemble, ode_method_cache, timestep_, timesteps_,
                            timesteps_ensemble_)


def get_state(stepper):
    """solver.jl:95-98"""
    return dict(u=stepper.u, temp=stepper.temp, t=stepper.t, n=stepper.n)


def get_cfl_timestep_(buf, u, setup):
    """Get proposed maximum time step for convection and diffusion terms (solver.jl:101-125).
    `buf` is accepted for signature parity; the reduction scratch is internal.  Blocking."""
    out = C.c_double()
    _lib.call("ins_cfl_timestep_f64", setup.handle, setup.Re, setup.ptr(u, True), C.byref(out), setup.stream)
    return out.value


def _is_float32_run(ustart, tempstart, psolver, cache):
    """True if `ustart` selects the Float32 family.  A solver, cache or temperature of the other precision is refused (TypeError), never cast."""
    from . import f32

    is32 = getattr(ustart, "dtype", None) == torch.float32
    mine, other = ("float32", "float64") if is32 else ("float64", "float32")
    if tempstart is not None and (getattr(tempstart, "dtype", None) == torch.float32) != is32:
        raise TypeError(f"solve_unsteady: a {mine} ustart with a {other} tempstart: give both fields in one precision")
    if psolver is not None and isinstance(psolver, f32.psolver_spectral32) != is32:
        raise TypeError(f"solve_unsteady: a {mine} ustart with a {other} psolver (float32 fields: f32.default_psolver32 / f32.psolver_wrap32; "
                        "float64 fields: default_psolver and its kin)")
    if cache is not None and isinstance(cache, f32.ERKCache32) != is32:
        raise TypeError(f"solve_unsteady: a {mine} ustart with a {other} cache (float32 fields: f32.ERKCache32; float64 fields: ode_method_cache)")
    return is32


def _solve_unsteady32(*, setup, tlims, u, temp, method, psolver, Δt, Δt_min, cfl, n_adapt_Δt, docopy, processors, θ, cache):
    """solve_unsteady (solver.jl:18-92) with T = Float32: the loop of the fp64 path on `f32.timestep32_` / `f32.timesteps32_` and
    `f32.get_cfl_timestep32_`.  `t` and `n` are kept on the host in double; `temp`, `θ`, a steady body force and the Smagorinsky closure go to the
    step functions as they are (what those refuse is refused here)."""
    from . import f32

    method = method or RKMethods.RK44()
    if isinstance(method, LMWray3):
        raise NotImplementedError("solve_unsteady on float32 fields runs the explicit Runge-Kutta methods (LMWray3: float64 fields)")
    if (temp is None) != (setup.temperature is None):
        raise ValueError("a temperature field needs setup.temperature (temperature_equation) and vice versa")
    psolver = psolver or f32.default_psolver32(setup)
    cache = cache or f32.ERKCache32(method, setup, psolver)
    if cache.psolver is not psolver:
        raise ValueError("cache was created for a different psolver")
    processors = processors or {}
    if docopy:
        u = copyfield(u)
        temp = None if temp is None else copyfield(temp)
    tstart, tend = tlims
    stepper = create_stepper(method, setup=setup, psolver=psolver, u=u, temp=temp, t=tstart)
    state = {"value": get_state(stepper)}
    initialized = {k: v.initialize(lambda: state["value"]) for k, v in processors.items()}

    def advance(k, Δt, t_new=None):
        if k > 1:
            f32.timesteps32_(cache, u, Δt, k, temp=temp, θ=θ)
        else:
            f32.timestep32_(cache, u, Δt, temp=temp, θ=θ)
        stepper.t = stepper.t + k * Δt if t_new is None else t_new
        stepper.n += k
        state["value"] = get_state(stepper)
        for v in processors.values():
            if hasattr(v, "on_step"):
                v.on_step(state["value"])

    if Δt is None:
        while stepper.t < tend:
            if stepper.n % n_adapt_Δt == 0:
                Δt = cfl * f32.get_cfl_timestep32_(u, setup)
                Δt = Δt if Δt_min is None else max(Δt, Δt_min)
            last = Δt >= tend - stepper.t  # the step that is clipped to tend lands on it exactly
            Δt = min(Δt, tend - stepper.t)
            advance(1, Δt, tend if last else None)
    else:
        nstep = int(round((tend - tstart) / Δt))
        Δt = (tend - tstart) / nstep
        if not processors:  # nobody looks at the intermediate states: the whole loop is one native call
            advance(nstep, Δt)
        else:  # the batching of the fp64 path: the steps between the multiples of gcd(nupdate...) run as one native call
            g = 0
            for v in processors.values():
                g = math.gcd(g, int(getattr(v, "nupdate", 1)))
            if g <= 1 or os.environ.get("INS_NO_PROCESSOR_BATCH"):
                g = 1
            done = 0
            while done < nstep:
                k = min(g - (stepper.n % g), nstep - done)
                advance(k, Δt)
                done += k
    outputs = {k: processors[k].finalize(initialized[k], lambda: state["value"]) for k in processors}
    return (stepper.u, stepper.temp, stepper.t), outputs


def solve_unsteady(*, setup, tlims, ustart, tempstart=None, method=None, psolver=None, Δt=None, Δt_min=None,
                   cfl=0.9, n_adapt_Δt=1, docopy=True, processors=None, θ=None, cache=None):
    """Solve unsteady problem using `method` (solver.jl:18-92).

    `processors` is a dict name -> object with `initialize(state_getter)` / `finalize(init, state_getter)`
    and an optional `on_step(state)`; returns `((u, temp, t), outputs)` like the reference.

    A `torch.float32` `ustart` (and `tempstart`) selects the Float32 family (`T = Float32` of the reference; f32.py): the default solver is
    `f32.default_psolver32(setup)`, the default cache `f32.ERKCache32(method, setup, psolver)`; mixing precisions raises TypeError."""
    if _is_float32_run(ustart, tempstart, psolver, cache):
        return _solve_unsteady32(setup=setup, tlims=tlims, u=ustart, temp=tempstart, method=method, psolver=psolver, Δt=Δt, Δt_min=Δt_min, cfl=cfl,
                                 n_adapt_Δt=n_adapt_Δt, docopy=docopy, processors=processors, θ=θ, cache=cache)
    method = method or RKMethods.RK44()
    psolver = psolver or default_psolver(setup)
    cache = cache or ode_method_cache(method, setup, psolver)
    processors = processors or {}
    if docopy:
        ustart = copyfield(ustart)
        tempstart = None if tempstart is None else copyfield(tempstart)
    tstart, tend = tlims
    isadaptive = Δt is None
    stepper = create_stepper(method, setup=setup, psolver=psolver, u=ustart, temp=tempstart, t=tstart)
    state = {"value": get_state(stepper)}
    initialized = {k: v.initialize(lambda: state["value"]) for k, v in processors.items()}

    def fire():
        state["value"] = get_state(stepper)
        for v in processors.values():
            if hasattr(v, "on_step"):
                v.on_step(state["value"])

    if isadaptive:
        while stepper.t < tend:
            if stepper.n % n_adapt_Δt == 0:
                Δt = cfl * get_cfl_timestep_(None, stepper.u, setup)
                Δt = Δt if Δt_min is None else max(Δt, Δt_min)
            Δt = min(Δt, tend - stepper.t)
            stepper = timestep_(method, stepper, Δt, θ=θ, cache=cache)
            fire()
    else:
        nstep = int(round((tend - tstart) / Δt))
        Δt = (tend - tstart) / nstep
        if not processors:  # nobody looks at the intermediate states: the whole loop is one native call
            stepper = timesteps_(method, stepper, Δt, nstep, θ=θ, cache=cache)
            fire()
        else:
            # processors that act every `nupdate` steps only (timelogger, fieldsaver, vtk_writer say so; a user-made processor has nupdate = 1) never look at
            # the states in between: those steps run as one native call (chained steps), and the state fires at the multiples of gcd(nupdate...) — every
            # step a processor acts on is among them.  INS_NO_PROCESSOR_BATCH=1: one call and one state update per step, as the reference's loop.
            g = 0
            for v in processors.values():
                g = math.gcd(g, int(getattr(v, "nupdate", 1)))
            if g <= 1 or os.environ.get("INS_NO_PROCESSOR_BATCH"):
                g = 1
            done = 0
            while done < nstep:
                k = min(g - (stepper.n % g), nstep - done)
                stepper = timesteps_(method, stepper, Δt, k, θ=θ, cache=cache) if k > 1 else timestep_(method, stepper, Δt, θ=θ, cache=cache)
                done += k
                fire()
    outputs = {k: processors[k].finalize(initialized[k], lambda: state["value"]) for k in processors}
    return (stepper.u, stepper.temp, stepper.t), outputs


def solve_unsteady_ensemble(*, cache, U, tlims, Δt=None, Δt_min=None, cfl=0.9, n_adapt_Δt=1, docopy=True, observe=None, nupdate=1):
    """The loop of `solve_unsteady` for all members of the ensemble field `U` of an `EnsembleCache`, with ONE Δt shared by the members.

    Fixed Δt: `nstep = round((tend - tstart) / Δt)` steps; the steps between the multiples of `nupdate` run as one `timesteps_ensemble_` call.
    `Δt=None`: every `n_adapt_Δt` steps `Δt = cfl · get_cfl_timestep_ensemble(cache, U)` (the smallest CFL step of any member; one host read), raised
    to `Δt_min` when given; the last step is clipped to `tend`.  The `n_adapt_Δt` steps of one Δt run as one native call when all of them fit before
    `tend` (and no multiple of `nupdate` lies inside them), otherwise step by step.
    `observe(U, t, n)` is called at n = 0 and at every multiple of `nupdate`.  `t` accumulates as `solve_unsteady` accumulates it for the same calls.
    Returns `((U, t), Δts)` with the list of the Δt of every step.  `U` passes the checks of `timesteps_ensemble_`."""
    _ensemble_ustride(cache, U)  # the checks of timesteps_ensemble_, before anything is copied or launched
    n_adapt_Δt, nupdate = int(n_adapt_Δt), int(nupdate)
    if n_adapt_Δt < 1 or nupdate < 1:
        raise ValueError("n_adapt_Δt and nupdate are positive")
    if docopy:
        V = vectorfields(cache.setup, cache.B)
        V.copy_(U)
        U = V
    tstart, tend = tlims
    c_end = cache.method.c[-1]
    t, n, Δts = tstart, 0, []

    def advance(k, Δt):
        nonlocal t, n
        timesteps_ensemble_(cache, U, t, Δt, k)
        t = t + (c_end * Δt if k == 1 else k * c_end * Δt)  # timestep_ / timesteps_
        n += k
        Δts.extend([Δt] * k)
        if observe is not None and n % nupdate == 0:
            observe(U, t, n)

    if observe is not None:
        observe(U, t, n)
    if Δt is None:
        while t < tend:
            if n % n_adapt_Δt == 0:
                Δt = cfl * get_cfl_timestep_ensemble(cache, U)
                Δt = Δt if Δt_min is None else max(Δt, Δt_min)
            Δt = min(Δt, tend - t)
            k = n_adapt_Δt - n % n_adapt_Δt  # steps this Δt still holds for
            if observe is not None:
                k = min(k, nupdate - n % nupdate)
            if k > 1 and t + k * c_end * Δt < tend:
                advance(k, Δt)
            else:
                advance(1, Δt)
    else:
        nstep = int(round((tend - tstart) / Δt))
        Δt = (tend - tstart) / nstep
        g = nupdate if observe is not None else nstep
        done = 0
        while done < nstep:
            k = min(g - n % g, nstep - done)
            advance(k, Δt)
            done += k
    return (U, t), Δts
