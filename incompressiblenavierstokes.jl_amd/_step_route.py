"""What the steppers ask of a setup before a step, asked once: `classify` reads the facts a stage loop is chosen by and a refusal is worded on,
`route` maps them to the one launch sequence `timestep_` / `timesteps_` run (DESIGN.md "Step routes" has the table).  The Float32 stepper (f32.py) and
the differentiable steps and rollouts (autodiff.py, autodiff32.py, _autodiff_core.check_rollout) take their decisions from the same record.

Device-free: attributes of the setup are read, nothing is called on it, so the stand-in setups of the CPU tests classify like real ones."""
import enum
import os
from typing import NamedTuple

import numpy as np

from .boundary_conditions import DirichletBC, HaloBC


class Force(enum.Enum):
    NONE, STEADY, UNSTEADY = range(3)


class Closure(enum.Enum):
    NONE, LIBRARY, USER = range(3)  # LIBRARY: made by smagorinsky_closure / smagorinsky_closure32 (the native loops can run it); USER: any other callable


class Route(enum.Enum):
    NATIVE = "ins_rk_step_f64 / ins_rk_steps_f64"
    NATIVE_BC = "ins_rk_step_bc_f64"
    NATIVE_EXT = "ins_rk_step_ext_f64"
    HOST_ERK = "host stage loop"
    HOST_LMWRAY3 = "host low-storage loop"


class Facts(NamedTuple):
    bc_u_callable: bool  # callable velocity Dirichlet data
    bc_temp_callable: bool  # callable temperature Dirichlet data (of the setup's temperature equation, with or without a field)
    force: Force
    slab: bool  # a HaloBC side
    closure: Closure
    closure_dtype: object  # LIBRARY: torch.float64 / torch.float32 (None: the stand-in of `_autodiff_core.native_closure`)
    closure_mine: bool  # LIBRARY: made for this setup
    closure_ad: object  # "ad" / "ad32": the differentiable Smagorinsky closure of that module for this setup (a USER closure to the step functions)
    theta_scalar: bool
    has_temp: bool


# ---- the markers on a closure model: set and read here only
def mark_library_closure(closure, setup, dtype=None):
    closure._ins_closure, closure._ins_setup, closure._ins_dtype = "smagorinsky", setup, dtype
    return closure


def mark_ad_closure(closure, name, setup):
    closure._ad_smagorinsky = (name, setup)
    return closure


def classify(setup, temp=None, θ=None):
    m = setup.closure_model
    library = getattr(m, "_ins_closure", None) == "smagorinsky"
    tag = getattr(m, "_ad_smagorinsky", None)
    T = setup.temperature
    return Facts(
        bc_u_callable=bool(setup.needs_bc_planes),
        bc_temp_callable=T is not None and any(isinstance(bc, DirichletBC) and callable(bc.u) for side in T.boundary_conditions for bc in side),
        force=Force.NONE if setup.bodyforce is None else Force.STEADY if setup.issteadybodyforce else Force.UNSTEADY,
        slab=any(isinstance(bc, HaloBC) for side in setup.boundary_conditions for bc in side),
        closure=Closure.NONE if m is None else Closure.LIBRARY if library else Closure.USER,
        closure_dtype=getattr(m, "_ins_dtype", None) if library else None,
        closure_mine=library and getattr(m, "_ins_setup", None) is setup,
        closure_ad=tag[0] if tag is not None and tag[1] is setup else None,
        theta_scalar=np.isscalar(θ),
        has_temp=temp is not None)


def steady_force(setup):
    """The stored field of a steady body force, or None."""
    return setup.bodyforce if classify(setup).force is Force.STEADY else None


def smagorinsky_of(facts, name, dtype):
    """True when the closure model is the library's Smagorinsky closure of this setup in the precision `dtype`: the fused one, or the differentiable
    one of the module `name` (`ad` / `ad32`)."""
    return (facts.closure_mine and facts.closure_dtype == dtype) or facts.closure_ad == name


def host_loop_requested():
    """INS_HOST_STAGE_LOOP, read per call: the escape to the host stage loops (tests set it in the middle of a process)."""
    return bool(os.environ.get("INS_HOST_STAGE_LOOP"))


def route(lmwray3, f, host_loop):
    """The launch sequence of one step.  `lmwray3`: the method is the low-storage scheme (natively it runs as the explicit RK method it is)."""
    plain = not (f.has_temp or f.closure is not Closure.NONE or f.force is Force.UNSTEADY or f.bc_u_callable)
    # the extended loop: a temperature with constant data, the library closure of this setup with a scalar θ, nothing that needs the host between kernels
    ext = not (f.bc_u_callable or f.force is Force.UNSTEADY or (f.has_temp and f.bc_temp_callable)
               or (f.closure is not Closure.NONE and not (f.closure_mine and f.theta_scalar)))
    if lmwray3:
        if host_loop or not (plain or ext):
            return Route.HOST_LMWRAY3
        return Route.NATIVE if plain else Route.NATIVE_EXT
    if plain:
        return Route.NATIVE  # (the escape does not reach it: with nothing between the kernels the host loop has nothing to show)
    if host_loop:
        return Route.HOST_ERK
    if f.bc_u_callable and not f.has_temp and f.closure is Closure.NONE and f.force is not Force.UNSTEADY:
        return Route.NATIVE_BC
    return Route.NATIVE_EXT if ext else Route.HOST_ERK


def step_route(lmwray3, setup, temp, θ):
    return route(lmwray3, classify(setup, temp, θ), host_loop_requested())
