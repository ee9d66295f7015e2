"""Host mirror of the `_f32` entry-point family (include/ins_hip.h; csrc/ins_f32.hip, csrc/ins_f32g.hip): the reference with `T = Float32`
(docs/src/manual/precision.md:3-16, examples/DecayingTurbulence3D.jl:16): all-periodic uniform boxes on the spectral solver, every other grid
(walls, symmetric / pressure sides, stretched spacings; constant boundary data) on `psolver_wrap32` around an fp64 solver.  The temperature equation
(csrc/ins_temp32.hip; examples/RayleighBenard3D.jl:16) rides on both: its operators, and `timestep32_` / `timesteps32_` with `temp=`.  So do the
Smagorinsky closure (csrc/ins_smagforce32.hip: `smagorinsky_closure32`, `θ=` of the step functions) and a steady `setup.bodyforce`.
`solve_unsteady` with a float32 `ustart` drives all of it (solver.py), with `get_cfl_timestep32_` for the adaptive Δt and the float observers
(csrc/ins_fields32.hip) behind the processors.

Fields are torch.float32 tensors in the reference layout; `setup` is the ordinary (fp64-metric) Setup."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._step_route import Closure, Force, classify, mark_library_closure
from .setup import _fortran_strides


def _alloc32(setup, shape):
    t = torch.zeros(tuple(reversed(shape)), dtype=torch.float32, device=setup.device)
    return t.permute(*reversed(range(len(shape))))


def scalarfield32(setup):
    return _alloc32(setup, setup.grid.N)


def vectorfield32(setup):
    return _alloc32(setup, setup.grid.N + (setup.grid.dimension,))


def to_f32(setup, f):
    """Round a float64 field (torch, reference layout) or a numpy array of field shape to a float32 device field."""
    out = _alloc32(setup, tuple(f.shape))
    out.copy_(f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f)).to(setup.device))
    return out


def _ptr(setup, f, ncomp):
    shape = setup.grid.N + ((ncomp,) if ncomp else ())
    if not isinstance(f, torch.Tensor) or f.dtype != torch.float32:
        raise TypeError("the _f32 family takes float32 torch tensors")
    if f.device != setup.device or tuple(f.shape) != shape or tuple(f.stride()) != _fortran_strides(shape):
        raise ValueError(f"field must live on {setup.device} with shape {shape} and column-major strides")
    return C.c_void_p(f.data_ptr())


def _constant_bc_only(setup):
    if classify(setup).bc_u_callable:
        raise NotImplementedError("the _f32 family takes constant boundary data (callable DirichletBC values: use the fp64 entry points)")


def apply_bc_u32_(u, setup, dudt=False):
    """apply_bc_u!(u, t, setup; dudt) with T = Float32 and constant boundary data: with `dudt` the field is a time derivative and the Dirichlet
    data contributes zero."""
    _constant_bc_only(setup)
    _lib.call("ins_apply_bc_u_dudt_f32" if dudt else "ins_apply_bc_u_f32", setup.handle, _ptr(setup, u, setup.grid.dimension), setup.stream)
    return u


def apply_bc_p32_(p, setup):
    _lib.call("ins_apply_bc_p_f32", setup.handle, _ptr(setup, p, 0), setup.stream)
    return p


def momentum32_(F, u, setup, temp=None):
    """momentum!(F, u, temp, t, setup) with T = Float32 (operators.jl:967-976): with `temp` the gravity term is added."""
    D = setup.grid.dimension
    _lib.call("ins_momentum_f32", setup.handle, float(1.0 / setup.Re), _ptr(setup, u, D), _ptr(setup, F, D), setup.stream)
    if temp is not None:
        gravity32_(F, temp, setup)
    return F


# ---- temperature equation (csrc/ins_temp32.hip): the Float32 twins of operators.apply_bc_temp_ ... gravity_, constant boundary data
def _temp_desc(setup):
    """ins_temperature_desc_t of setup.temperature (the one `time_steppers._temperature_desc` builds); callable Dirichlet data is refused."""
    from .time_steppers import _temperature_desc

    if setup.temperature is None:
        raise ValueError("the setup has no temperature equation (Setup(temperature=temperature_equation(...)))")
    if classify(setup).bc_temp_callable:
        raise NotImplementedError("the _f32 family takes constant boundary data (callable temperature DirichletBC values: use the fp64 "
                                  "entry points)")
    return _temperature_desc(setup)


def apply_bc_temp32_(temp, setup):
    """apply_bc_temp!(temp, t, setup) with T = Float32, in place (boundary_conditions.jl:236-246)."""
    desc = _temp_desc(setup)
    vals = (C.c_float * 6)(*[desc.val[q] for q in range(6)])
    _lib.call("ins_apply_bc_temp_f32", setup.handle, desc.bc, vals, _ptr(setup, temp, 0), setup.stream)
    return temp


def convection_diffusion_temp32_(c, u, temp, setup):
    """operators.jl:712-737 with T = Float32 (adds to c)"""
    _lib.call("ins_convection_diffusion_temp_f32", setup.handle, float(_temp_desc(setup).a4), _ptr(setup, u, setup.grid.dimension), _ptr(setup, temp, 0),
              _ptr(setup, c, 0), setup.stream)
    return c


def dissipation32_(diss, diff, u, setup):
    """operators.jl:791-814 with T = Float32 (adds to diss; `diff` is scratch: it receives diffusion(u), zeros off the degrees of freedom)"""
    D = setup.grid.dimension
    _lib.call("ins_dissipation_f32", setup.handle, float(1.0 / setup.Re), float(_temp_desc(setup).diss_coef), _ptr(setup, u, D), _ptr(setup, diff, D),
              _ptr(setup, diss, 0), setup.stream)
    return diss


def gravity32_(F, temp, setup):
    """operators.jl:914-931 with T = Float32 (adds to F)"""
    desc = _temp_desc(setup)
    _lib.call("ins_gravity_f32", setup.handle, int(desc.gdir), float(desc.a2), _ptr(setup, temp, 0), _ptr(setup, F, setup.grid.dimension), setup.stream)
    return F


def temperaturefield32(setup, tempfunc):
    """temperaturefield(setup, tempfunc) with T = Float32 (initializers.jl:48-57): `tempfunc(x, y[, z])` on the pressure points (evaluated in double on
    the host, rounded once), then the ghost fill."""
    g = setup.grid
    D = g.dimension
    host = np.zeros(g.N, dtype=np.float64, order="F")
    xs = []
    for be in range(D):
        lo, hi = g.Ip[be]
        shape = [1] * D
        shape[be] = hi - lo
        xs.append(np.asarray(g.xp[be][lo:hi]).reshape(shape))
    sl = tuple(slice(lo, hi) for lo, hi in g.Ip)
    host[sl] = np.broadcast_to(tempfunc(*xs), tuple(hi - lo for lo, hi in g.Ip))
    return apply_bc_temp32_(to_f32(setup, host), setup)


class psolver_spectral32:
    """psolver_spectral(setup) with T = Float32 (pressure.jl:289-351)."""

    def __init__(self, setup):
        self.setup = setup
        self._handle = C.c_void_p()
        _lib.call("ins_poisson_spectral_create_f32", setup.handle, C.byref(self._handle))

    @property
    def handle(self):
        return self._handle

    def __call__(self, p):
        _lib.call("ins_poisson_solve_f32", self._handle, _ptr(self.setup, p, 0), self.setup.stream)
        return p

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                _lib.load().ins_poisson_destroy_f32(h)
            except Exception:
                pass


class psolver_wrap32(psolver_spectral32):
    """psolver_direct(setup) / psolver_cg(setup) / psolver_spectral(setup) with T = Float32 on any grid (pressure.jl:85-154, 209-351): a Float32 solver
    around the fp64 solver `psolver64` (default: the setup's default_psolver) — right-hand side in double, fp64 solve, pressure rounded once."""

    def __init__(self, setup, psolver64=None):
        from .pressure import default_psolver

        self.setup = setup
        self.psolver64 = psolver64 if psolver64 is not None else default_psolver(setup)  # kept alive: the native handle borrows it
        self._handle = C.c_void_p()
        _lib.call("ins_poisson_wrap_f32", setup.handle, self.psolver64.handle, C.byref(self._handle))


def default_psolver32(setup):
    """default_psolver(setup) with T = Float32 (pressure.jl:85-98): spectral on all-periodic uniform boxes, direct elsewhere."""
    from .pressure import default_psolver, psolver_spectral

    ps64 = default_psolver(setup)
    if isinstance(ps64, psolver_spectral):
        del ps64
        return psolver_spectral32(setup)
    return psolver_wrap32(setup, ps64)


def project32_(u, setup, psolver, p):
    """project!(u, setup; psolver, p) with T = Float32 (pressure.jl:69-82)."""
    D = setup.grid.dimension
    _lib.call("ins_project_f32", setup.handle, psolver.handle, _ptr(setup, u, D), _ptr(setup, p, 0), setup.stream)
    return u


# ---- pullbacks (csrc/ins_adjoint32.hip): the exact transposes of the operators above on the whole padded float arrays
def divergence_adjoint32_(ubar, φ, setup):
    """operators.jl:127-145 (adds Dᵀφ to ubar)"""
    _lib.call("ins_divergence_adjoint_f32", setup.handle, _ptr(setup, φ, 0), _ptr(setup, ubar, setup.grid.dimension), setup.stream)
    return ubar


def pressuregradient_adjoint32_(pbar, φ, setup):
    """operators.jl:180-199 (adds Gᵀφ to pbar)"""
    _lib.call("ins_pressuregradient_adjoint_f32", setup.handle, _ptr(setup, φ, setup.grid.dimension), _ptr(setup, pbar, 0), setup.stream)
    return pbar


def momentum_pullback32_(ubar, φbar, u, setup, accumulate=False):
    """Pullback of momentum32_ at the ghost-filled `u` (convection + diffusion in one launch): ubar = J(u)ᵀφbar, or ubar += J(u)ᵀφbar with `accumulate`."""
    D = setup.grid.dimension
    _lib.call("ins_momentum_pullback_f32", setup.handle, float(1.0 / setup.Re), _ptr(setup, u, D), _ptr(setup, φbar, D), _ptr(setup, ubar, D),
              int(bool(accumulate)), setup.stream)
    return ubar


def apply_bc_u_pullback32_(φbar, setup):
    """boundary_conditions.jl:169-206, in place: the transpose of apply_bc_u32_ (constant boundary data)."""
    _lib.call("ins_apply_bc_u_pullback_f32", setup.handle, _ptr(setup, φbar, setup.grid.dimension), setup.stream)
    return φbar


def apply_bc_p_pullback32_(φbar, setup):
    """boundary_conditions.jl:208-230, in place: the transpose of apply_bc_p32_."""
    _lib.call("ins_apply_bc_p_pullback_f32", setup.handle, _ptr(setup, φbar, 0), setup.stream)
    return φbar


def project_pullback32_(φbar, setup, psolver, pwork):
    """Pullback of project32_ in place (pressure.jl:52-82, 15-19): the transpose of what project32_ does to the whole padded array with this
    kind of solver (include/ins_hip.h); `pwork` is a float32 scalar field of scratch."""
    D = setup.grid.dimension
    _lib.call("ins_project_pullback_f32", setup.handle, psolver.handle, _ptr(setup, φbar, D), _ptr(setup, pwork, 0), setup.stream)
    return φbar


# ---- temperature pullbacks (csrc/ins_temp_adjoint32.hip): the Float32 twins of operators.apply_bc_temp_pullback_ ... temperature_pullback_, the exact
# transposes of the Float32 temperature operators above on the whole padded float arrays.  The scalars come from _temp_desc(setup): callable
# temperature Dirichlet data raises NotImplementedError there.
def apply_bc_temp_pullback32_(tempbar, setup):
    """boundary_conditions.jl:248-270, in place: the transpose of the linear part of apply_bc_temp32_ (the Dirichlet values do not enter)."""
    _lib.call("ins_apply_bc_temp_pullback_f32", setup.handle, _temp_desc(setup).bc, _ptr(setup, tempbar, 0), setup.stream)
    return tempbar


def gravity_adjoint32_(tempbar, φbar, setup):
    """operators.jl:892-908 (adds (α2 avg)ᵀ φbar[..., gdir] to tempbar)"""
    desc = _temp_desc(setup)
    _lib.call("ins_gravity_adjoint_f32", setup.handle, int(desc.gdir), float(desc.a2), _ptr(setup, φbar, setup.grid.dimension), _ptr(setup, tempbar, 0),
              setup.stream)
    return tempbar


def convection_diffusion_temp_adjoint32_(ubar, tempbar, cbar, u, temp, setup):
    """operators.jl:712-737 at the ghost-filled (u, temp): adds (∂c/∂u)ᵀ cbar to `ubar` and (∂c/∂temp)ᵀ cbar to `tempbar`; either may be
    None to skip that half.  Returns (ubar, tempbar)."""
    D = setup.grid.dimension
    _lib.call("ins_convection_diffusion_temp_adjoint_f32", setup.handle, float(_temp_desc(setup).a4), _ptr(setup, u, D), _ptr(setup, temp, 0),
              _ptr(setup, cbar, 0), _ptr_or_null(setup, ubar, D), _ptr_or_null(setup, tempbar, 0), setup.stream)
    return ubar, tempbar


def dissipation_adjoint32_(ubar, cbar, u, setup):
    """operators.jl:791-814 at the ghost-filled `u` (adds J(u)ᵀ cbar to ubar; diffusion(u) is recomputed in the kernel, no scratch field)"""
    D = setup.grid.dimension
    _lib.call("ins_dissipation_adjoint_f32", setup.handle, float(1.0 / setup.Re), float(_temp_desc(setup).diss_coef), _ptr(setup, u, D),
              _ptr(setup, cbar, 0), _ptr(setup, ubar, D), setup.stream)
    return ubar


def temperature_pullback32_(ubar, tempbar, Fbar, cbar, u, temp, setup):
    """One Runge-Kutta stage's temperature-coupled pullback in one launch: tempbar = gravityᵀ Fbar + (∂c/∂temp)ᵀ cbar (overwritten),
    ubar += (∂c/∂u)ᵀ cbar + dissipationᵀ cbar (the latter with `dodissipation`), on top of what `momentum_pullback32_` wrote.
    Returns (ubar, tempbar)."""
    D = setup.grid.dimension
    desc = _temp_desc(setup)
    _lib.call("ins_temperature_pullback_f32", setup.handle, C.byref(desc), float(1.0 / setup.Re), _ptr(setup, u, D), _ptr(setup, temp, 0),
              _ptr(setup, Fbar, D), _ptr(setup, cbar, 0), _ptr(setup, ubar, D), _ptr(setup, tempbar, 0), setup.stream)
    return ubar, tempbar


# ---- tensor-basis closure (csrc/ins_tensorclosure32.hip): the Float32 twins of operators.tensorinvariants_ ... divoftensor_adjoint_
def _tb_sizes(setup):
    """(nb, nv, ns): basis tensors, invariants, stored entries of a symmetric tensor."""
    D = setup.grid.dimension
    return ((3, 2) if D == 2 else (11, 5)) + (D * (D + 1) // 2,)


def nfield32(setup, ncomp):
    """A zero float32 field of `ncomp` scalar fields, N + (ncomp,)."""
    return _alloc32(setup, setup.grid.N + (ncomp,))


def tensorfield32(setup):
    """Symmetric tensor field: D(D+1)/2 float32 scalar fields [xx, yy, (zz), xy, (xz, yz)] (operators.tensorfield)."""
    return nfield32(setup, _tb_sizes(setup)[2])


def _ptr_or_null(setup, f, ncomp):
    return None if f is None else _ptr(setup, f, ncomp)


def tensorinvariants32_(V, u, setup):
    """The invariants of the tensor basis (tensorbasis.jl:49-50, 70-74) with T = Float32: writes `V`, N + (nv,), on Ip."""
    _lib.call("ins_tensorinvariants_f32", setup.handle, _ptr(setup, u, setup.grid.dimension), _ptr(setup, V, _tb_sizes(setup)[1]), setup.stream)
    return V


def tensorclosure_stress32_(τ, u, a, setup):
    """τ = Σ_i a_i B_i(u) on Ip (tensorbasis.jl:59-69, 137-146) with T = Float32, without storing B: `a` is N + (nb,), `τ` a `tensorfield32`."""
    nb, _, ns = _tb_sizes(setup)
    _lib.call("ins_tensorclosure_stress_f32", setup.handle, _ptr(setup, u, setup.grid.dimension), _ptr(setup, a, nb), _ptr(setup, τ, ns), setup.stream)
    return τ


def tensorclosure_pullback32_(ubar, abar, τbar, Vbar, u, a, setup, accumulate=False):
    """One backward for `tensorclosure_stress32_` and `tensorinvariants32_`: abar_i = <τbar, B_i> (overwritten), ubar = J_τ(u)ᵀτbar + J_V(u)ᵀVbar
    (overwritten, or added to with `accumulate`).  `Vbar` may be None; `abar`, `τbar` and `a` may be None together."""
    nb, nv, ns = _tb_sizes(setup)
    D = setup.grid.dimension
    _lib.call("ins_tensorclosure_pullback_f32", setup.handle, _ptr(setup, u, D), _ptr_or_null(setup, a, nb), _ptr_or_null(setup, τbar, ns),
              _ptr_or_null(setup, Vbar, nv), _ptr_or_null(setup, abar, nb), _ptr(setup, ubar, D), int(bool(accumulate)), setup.stream)
    return ubar


def divoftensor32_(s, σ, setup):
    """operators.jl:1158-1175, 1203-1236 with T = Float32, on the D(D+1)/2 symmetric fields."""
    _lib.call("ins_divoftensor_f32", setup.handle, _ptr(setup, σ, _tb_sizes(setup)[2]), _ptr(setup, s, setup.grid.dimension), setup.stream)
    return s


def divoftensor_adjoint32_(σbar, sbar, setup):
    """operators.jl:1186-1287 with T = Float32 (adds the transpose of divoftensor32_ applied to sbar to the symmetric fields σbar)."""
    _lib.call("ins_divoftensor_adjoint_f32", setup.handle, _ptr(setup, sbar, setup.grid.dimension), _ptr(setup, σbar, _tb_sizes(setup)[2]), setup.stream)
    return σbar


# ---- Smagorinsky closure (csrc/ins_smagforce32.hip): the Float32 twins of operators.smagtensor_ and operators.smagorinsky_closure
def smagtensor32_(σ, u, θ, setup):
    """operators.jl:1135-1150 with T = Float32: writes the `tensorfield32` σ on Ip."""
    _lib.call("ins_smagtensor_f32", setup.handle, float(θ), _ptr(setup, u, setup.grid.dimension), _ptr(setup, σ, _tb_sizes(setup)[2]), setup.stream)
    return σ


def smagorinsky_force32_(s, u, θ, setup, σ=None):
    """s = divoftensor(apply_bc_p(smagtensor(u, θ))) on the degrees of freedom (operators.jl:1284-1300) with T = Float32: one kernel where the
    grid allows it, else the three kernels with the `tensorfield32` σ as scratch (required there: `ins_smagorinsky_force_needs_sigma`)."""
    D = setup.grid.dimension
    _lib.call("ins_smagorinsky_force_f32", setup.handle, float(θ), _ptr(setup, u, D), _ptr_or_null(setup, σ, _tb_sizes(setup)[2]), _ptr(setup, s, D),
              setup.stream)
    return s


def smagorinsky_force_pullback32_(ubar, θbar, sbar, u, θ, setup, accumulate=False):
    """Pullback of `smagorinsky_force32_` at the ghost-filled float32 `u` (csrc/ins_smagpullback_kernels.h with T = float): ubar = (∂s/∂u)ᵀ sbar
    (overwritten, or added to with `accumulate`) and θbar += (∂s/∂θ)ᵀ sbar, `θbar` a 0-dim FLOAT64 device tensor the caller zeroes (the cells' terms are
    formed in float and summed in double), or None."""
    from .operators import _thetabar_ptr

    D = setup.grid.dimension
    _lib.call("ins_smagorinsky_force_pullback_f32", setup.handle, float(θ), _ptr(setup, u, D), _ptr(setup, sbar, D), _ptr(setup, ubar, D),
              int(bool(accumulate)), _thetabar_ptr(setup, θbar), setup.stream)
    return ubar, θbar


def smagorinsky_closure32(setup):
    """Create the Smagorinsky closure model `m(u, θ)` on float32 padded fields (operators.jl:1284-1300), marked like `smagorinsky_closure` so that
    `timestep32_` / `timesteps32_` run it inside the native stage loop (ins_rk_set_closure_f32)."""
    s = vectorfield32(setup)
    scratch = {}

    def closure(u, θ):
        σ = None
        if _lib.load().ins_smagorinsky_force_needs_sigma(setup.handle):  # answers for both precisions; asked per call: an option may switch the route
            if "σ" not in scratch:
                scratch["σ"] = tensorfield32(setup)
            σ = scratch["σ"]
        return smagorinsky_force32_(s, u, θ, setup, σ)

    return mark_library_closure(closure, setup, torch.float32)


def max_abs_divergence32(u, setup, psolver):
    out = C.c_float()
    _lib.call("ins_max_abs_divergence_f32", setup.handle, psolver.handle, _ptr(setup, u, setup.grid.dimension), C.byref(out), setup.stream)
    return float(out.value)


# ---- what solve_unsteady and the processors need of a float32 state (csrc/ins_fields32.hip): the Float32 twins of solver.get_cfl_timestep_ and of
# operators.vorticity_, interpolate_u_p_, interpolate_ω_p_, Qfield_
def get_cfl_timestep32_(u, setup):
    """Proposed maximum time step for the convection and diffusion terms (solver.jl:101-125) of the float32 field `u`: one pass over `u`, the
    convective quotients Δu / |u| in float, the diffusive bound in double on the host.  Blocking; returns a Python float."""
    out = C.c_float()
    _lib.call("ins_cfl_timestep_f32", setup.handle, float(setup.Re), _ptr(setup, u, setup.grid.dimension), C.byref(out), setup.stream)
    return float(out.value)


def _ncomp_ω(setup):
    return 0 if setup.grid.dimension == 2 else 3


def vorticity32_(ω, u, setup):
    """operators.jl:985-1020 with T = Float32 (2-D: a scalar field; 3-D: a vector field); `u` ghost-filled."""
    _lib.call("ins_vorticity_f32", setup.handle, _ptr(setup, u, setup.grid.dimension), _ptr(setup, ω, _ncomp_ω(setup)), setup.stream)
    return ω


def interpolate_u_p32_(up, u, setup):
    """operators.jl:1311-1326 with T = Float32 (writes Ip)"""
    D = setup.grid.dimension
    _lib.call("ins_interpolate_u_p_f32", setup.handle, _ptr(setup, u, D), _ptr(setup, up, D), setup.stream)
    return up


def interpolate_ω_p32_(ωp, ω, setup):
    """operators.jl:1336-1370 with T = Float32 (writes Ip)"""
    _lib.call("ins_interpolate_w_p_f32", setup.handle, _ptr(setup, ω, _ncomp_ω(setup)), _ptr(setup, ωp, _ncomp_ω(setup)), setup.stream)
    return ωp


def Qfield32_(Q, u, setup):
    """operators.jl:1440-1460 with T = Float32 (writes Ip)"""
    _lib.call("ins_qfield_f32", setup.handle, _ptr(setup, u, setup.grid.dimension), _ptr(setup, Q, 0), setup.stream)
    return Q


class ERKCache32:
    """ode_method_cache(method, setup) with T = Float32 (time_stepper_caches.jl:34-49)."""

    def __init__(self, method, setup, psolver):
        self.setup, self.psolver = setup, psolver
        A = np.ascontiguousarray(method.A, dtype=np.float64)
        c = np.ascontiguousarray(method.c, dtype=np.float64)
        self._handle = C.c_void_p()
        dp = C.POINTER(C.c_double)
        _constant_bc_only(setup)
        _lib.call("ins_rk_create_f32", setup.handle, psolver.handle, len(method.b), A.ctypes.data_as(dp), c.ctypes.data_as(dp), C.byref(self._handle))

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h:
            try:
                _lib.load().ins_rk_destroy_f32(h)
            except Exception:
                pass


def _set_temperature32(cache, temp):
    """Hand the temperature descriptor of the cache's setup to its native handle (once per cache)."""
    s = cache.setup
    if s.temperature is None:
        raise ValueError("timestep32_ with `temp` needs a setup with a temperature equation")
    desc = _temp_desc(s)
    if not getattr(cache, "_has_temp", False):
        _lib.call("ins_rk_set_temperature_f32", cache._handle, C.byref(desc))
        cache._has_temp = True
    return _ptr(s, temp, 0)


def _set_force_closure32(cache, θ):
    """Hand the steady body force and the Smagorinsky closure of the cache's setup to its native handle; True if the extended loop is needed.
    What the Float32 stage loop does not run is refused: it would otherwise be dropped from the step without a word."""
    s = cache.setup
    facts = classify(s, None, θ)
    if facts.force is Force.UNSTEADY:
        raise NotImplementedError("the _f32 family takes a steady body force (an unsteady one: the fp64 entry points, timestep_ / solve_unsteady)")
    f = s.bodyforce
    if getattr(cache, "_force_src", None) is not f:  # cast once per cache; the float32 field is kept alive here
        cache._force32 = to_f32(s, f) if f is not None else None
        _lib.call("ins_rk_set_bodyforce_f32", cache._handle, _ptr(s, cache._force32, s.grid.dimension) if f is not None else None)
        cache._force_src = f
    if facts.closure is Closure.NONE:
        kind, θ = 0, 0.0  # (a θ without a closure model has nothing to act on, as in timestep_)
    else:
        if not facts.closure_mine:
            raise NotImplementedError("the _f32 stage loop runs the library's Smagorinsky closure of this setup (smagorinsky_closure / "
                                      "smagorinsky_closure32); another closure_model: the fp64 entry points, or ad32.timestep with a torch closure")
        if θ is None:
            raise NotImplementedError("the setup has a closure_model: give its parameter as θ= (a scalar); without one the closure would be dropped "
                                      "(fp64 entry points: timestep_(..., θ=θ))")
        if not facts.theta_scalar:
            raise NotImplementedError("the _f32 stage loop takes a scalar θ (a tensor θ: ad32.timestep with ad32.smagorinsky_closure)")
        kind, θ = 1, float(θ)
    if getattr(cache, "_closure", (0, 0.0)) != (kind, θ):
        _lib.call("ins_rk_set_closure_f32", cache._handle, kind, θ)
        cache._closure = (kind, θ)
    return f is not None or kind != 0


def _steps32_(plain, ext, cache, u, Δt, nsteps, temp, θ):
    """The body of both step functions: the entry `plain`, or with a temperature, a steady body force or the closure the entry `ext`; `nsteps`
    (an argument of the multi-step entries only) as a tuple."""
    s = cache.setup
    ext_needed = _set_force_closure32(cache, θ)
    if temp is None and not ext_needed:
        _lib.call(plain, cache._handle, float(1.0 / s.Re), _ptr(s, u, s.grid.dimension), float(Δt), *nsteps, s.stream)
        return u
    tp = _set_temperature32(cache, temp) if temp is not None else None
    _lib.call(ext, cache._handle, float(1.0 / s.Re), _ptr(s, u, s.grid.dimension), tp, float(Δt), *nsteps, s.stream)
    return u if temp is None else (u, temp)


def timestep32_(cache, u, Δt, temp=None, θ=None):
    """One explicit RK step of the float32 field `u` in place (step_explicit_runge_kutta.jl:4-59); with `temp` (a float32 scalar field; the setup has a
    temperature equation) the temperature is advanced with it and (u, temp) is returned.  A steady `setup.bodyforce` and the library's Smagorinsky
    `setup.closure_model` with the scalar parameter `θ` join every stage force (operators.jl:873-880, 1294-1305)."""
    return _steps32_("ins_rk_step_f32", "ins_rk_step_ext_f32", cache, u, Δt, (), temp, θ)


def timesteps32_(cache, u, Δt, nsteps, temp=None, θ=None):
    """`nsteps` explicit RK steps of size Δt of the float32 field `u` in place: the fixed-Δt loop of solve_unsteady (solver.jl:74-83) as one native call;
    with `temp` and `θ` as `timestep32_`."""
    return _steps32_("ins_rk_steps_f32", "ins_rk_steps_ext_f32", cache, u, Δt, (int(nsteps),), temp, θ)
