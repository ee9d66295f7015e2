"""lib/NeuralClosure of the reference on this library: DNS-to-LES filters (filter.jl), filtered-DNS data generation (data_generation.jl),
closure wrappers and the CNN (closure.jl, cnn.jl), data loaders, a-priori / a-posteriori losses and the training loop (training.jl).
Exported as `ins_amd.neuralclosure`; the main names also from `ins_amd`.

The filters run in csrc/ins_filter.hip and, on float32 fields, csrc/ins_filter32.hip.  The network is torch (float64, or
float32 with `dtype=torch.float32`; a Float32 DNS is filtered, stored and trained on in Float32): a closure is a callable `m(u, θ)`; for a
`torch.nn.Module` built by `cnn`, θ is `None` (the module's own parameters, which a `torch.optim` optimiser updates in place) or a
dict name -> tensor as `torch.func.functional_call` takes it.

Array layouts.  Fields are the library's padded tensors `N + (D,)`.  Training arrays (`create_io_arrays`, `collocate`, `decollocate`, the
CNN) are `(n_1, …, n_D, D, nsample)`: interior volumes only, component, then sample — the reference's layout; the CNN permutes to torch's
`(nsample, channel, n_1, …, n_D)` internally.  Trajectories (`filtersaver`) are padded: `N + (D, nt)`.

`tensorclosure` is the symmetry tensor-basis model (tensorbasis.jl) on the fused kernels of csrc/ins_tensorclosure.hip.

Out of scope: FNO and group-equivariant layers, the symmetry errors (`rot2stag`), `gaussian_force`, JLD2 files (`filenames` writes `.npz`).
"""
import os
import time

import numpy as np
import torch

from . import _lib
from . import autodiff as ad
from . import f32
from .initializers import random_field
from .operators import apply_bc_u_, momentum_
from .pressure import default_psolver, project_
from .processors import Observable, processor
from .setup import Setup, scalarfield, to_numpy, vectorfield
from .solver import solve_unsteady
from .time_steppers import _PER_TRAJECTORY, RKMethods, create_stepper, ode_method_cache, timestep_

__all__ = ["AbstractFilter", "FaceAverage", "VolumeAverage", "reconstruct", "reconstruct_", "lesdatagen", "filtersaver", "create_les_data",
           "create_les_data_ensemble", "create_io_arrays", "wrappedclosure", "wrappedclosure_ensemble", "collocate", "decollocate", "cnn", "tensorclosure", "create_dataloader_prior", "create_dataloader_post",
           "create_loss_prior", "create_relerr_prior", "create_loss_post", "create_loss_post_ensemble", "create_relerr_post", "train"]


# ------------------------------------------------------------------------------------------------ filters (filter.jl)
def _interior_faces(setup, b):
    """Face coordinates of direction b without the ghost volumes."""
    x = np.asarray(setup.grid.x[b])
    left = 2 if setup.boundary_conditions[b][0].code == _lib.INS_BC_PRESSURE else 1
    return x[left:-1]


def dns_setup_of(setup_les, comp):
    """The fine grid a filter call refers to when the caller gives none (the reference's filters take `setup_les` only and read sizes off the
    arrays): every coarse volume split into `comp` equal parts, same boundary conditions.  Cached on `setup_les`."""
    cache = setup_les.__dict__.setdefault("_dns_setups", {})
    if comp not in cache:
        xs = []
        for b in range(setup_les.grid.dimension):
            x = _interior_faces(setup_les, b)
            fine = [x[:-1] + (x[1:] - x[:-1]) * (q / comp) for q in range(comp)]
            xs.append(np.append(np.stack(fine, axis=1).reshape(-1), x[-1]))
        cache[comp] = Setup(x=tuple(xs), boundary_conditions=setup_les.boundary_conditions, Re=setup_les.Re, device=setup_les.device)
    return cache[comp]


def _is32(f):
    return isinstance(f, torch.Tensor) and f.dtype == torch.float32


def _one_precision(fine, coarse, what):
    if isinstance(fine, torch.Tensor) and isinstance(coarse, torch.Tensor) and fine.dtype != coarse.dtype:
        raise TypeError(f"{what}: the fine field is {fine.dtype}, the coarse field {coarse.dtype}; a filter call takes one precision")


def _filter_ptrs(dns, fine, les, coarse, what):
    """Entry suffix and the two field pointers of a filter call, by the precision of the fields: float64 -> `_f64`, float32 -> `_f32`
    (csrc/ins_filter32.hip).  The two fields are of one precision (TypeError, raised before a setup is touched)."""
    _one_precision(fine, coarse, what)
    if _is32(fine):
        D = dns.grid.dimension
        return "f32", f32._ptr(dns, fine, D), f32._ptr(les, coarse, D)
    return "f64", dns.ptr(fine, True), les.ptr(coarse, True)


class AbstractFilter:
    """Discrete DNS filter (filter.jl:1-15): `Φ(v, u, setup_les, comp)` filters the DNS field `u` into the LES field `v` (only `Iu[α]` is
    written: ghosts are the caller's `apply_bc_u_`); `Φ(u, setup_les, comp)` allocates `v`.  `setup_dns` names the fine grid; without it
    the fine grid is `setup_les` subdivided (`dns_setup_of`).  float32 fields take the `_f32` kernels (float loads and stores, sums in double,
    one rounding) and the allocating forms return a `f32.vectorfield32`; `u` and `v` of different precisions: TypeError."""

    _entry = None

    def __call__(self, *args, setup_dns=None):
        if len(args) == 3:
            u, setup_les, comp = args
            v = f32.vectorfield32(setup_les) if _is32(u) else vectorfield(setup_les)
        elif len(args) == 4:
            v, u, setup_les, comp = args
        else:
            raise TypeError("Φ(u, setup_les, comp) or Φ(v, u, setup_les, comp)")
        _one_precision(u, v, "Φ(v, u, …)")
        dns = setup_dns or dns_setup_of(setup_les, int(comp))
        sfx, pu, pv = _filter_ptrs(dns, u, setup_les, v, "Φ(v, u, …)")
        _lib.call(f"ins_filter_{self._entry}_{sfx}", setup_les.handle, dns.handle, int(comp), pu, pv, setup_les.stream)
        return v

    def members(self, V, U, setup_les, comp, setup_dns=None):
        """`Φ(V[b], U[b], setup_les, comp)` for every member of the ensemble fields `U` (fine) and `V` (coarse), both `(B,) + N + (D,)` as `vectorfields`
        makes them, in ONE launch (`ins_filter_{face,volume}_members_f64`): member b is bitwise what the per-member call gives, only `Iu[α]` of every
        `V[b]` is written.  A state and its right-hand side that share a buffer (`UF = vectorfields(dns, 2 * B)`) are filtered by one call.  float64, 2-D;
        float32 tensors: TypeError, 3-D grids: NotImplementedError, both naming the per-member call.  Returns V."""
        from .time_steppers import _member_stride

        per_member = f"filter each member with {type(self).__name__}()(V[b], U[b], setup_les, comp)"
        if _is32(U) or _is32(V):
            raise TypeError(f"Φ.members(V, U, …): the member form of the filters runs float64 fields; {per_member} (float32 fields take the `_f32` kernels there)")
        dns = setup_dns or dns_setup_of(setup_les, int(comp))
        ustride = _member_stride(dns, U)
        vstride = _member_stride(setup_les, V, U.shape[0])
        lib = _lib.load()
        rc = getattr(lib, f"ins_filter_{self._entry}_members_f64")(setup_les.handle, dns.handle, int(comp), int(U.shape[0]), U.data_ptr(), ustride,
                                                                  V.data_ptr(), vstride, setup_les.stream)
        if rc == -4:  # INS_ERR_UNSUPPORTED: a 3-D grid, a volume average on a non-periodic grid
            raise NotImplementedError(f"Φ.members(V, U, …): {lib.ins_last_error().decode()}; {per_member}")
        _lib.check(rc)
        return V

    def pullback_(self, ubar, w, setup_les, comp, setup_dns=None):
        """ubar = Φᵀ w over the whole padded fine array."""
        _one_precision(ubar, w, "pullback_(ubar, w, …)")
        dns = setup_dns or dns_setup_of(setup_les, int(comp))
        sfx, pubar, pw = _filter_ptrs(dns, ubar, setup_les, w, "pullback_(ubar, w, …)")
        _lib.call(f"ins_filter_{self._entry}_pullback_{sfx}", setup_les.handle, dns.handle, int(comp), pw, pubar, setup_les.stream)
        return ubar

    def __repr__(self):
        return f"{type(self).__name__}()"


class FaceAverage(AbstractFilter):
    """Average fine grid velocity field over coarse volume face (filter.jl:17-46)."""

    _entry = "face"


class VolumeAverage(AbstractFilter):
    """Average fine grid velocity field over coarse volume (filter.jl:20-21, 82-116).  All-periodic grids."""

    _entry = "volume"


def reconstruct_(u, v, setup_dns, setup_les, comp):
    """Reconstruct DNS velocity `u` from LES velocity `v` (filter.jl:48-76): writes the fine interior.  float64 or float32 fields."""
    sfx, pu, pv = _filter_ptrs(setup_dns, u, setup_les, v, "reconstruct_(u, v, …)")
    _lib.call(f"ins_reconstruct_{sfx}", setup_dns.handle, setup_les.handle, int(comp), pv, pu, setup_les.stream)
    return u


def reconstruct(v, setup_dns, setup_les, comp):
    """filter.jl:78-80"""
    return reconstruct_(f32.vectorfield32(setup_dns) if _is32(v) else vectorfield(setup_dns), v, setup_dns, setup_les, comp)


# ------------------------------------------------------------------------------------------------ data generation (data_generation.jl)
def _ops(single):
    """The operator chain of the data generation in one precision: (vectorfield, scalarfield, bc_u(u, t, setup, dudt), momentum(F, u, t, setup),
    project(u, setup, psolver, p)).  float32: the `_f32` family (f32.py), constant boundary data."""
    if single:
        return (f32.vectorfield32, f32.scalarfield32, lambda u, t, s, dudt=False: f32.apply_bc_u32_(u, s, dudt=dudt),
                lambda F, u, t, s: f32.momentum32_(F, u, s), f32.project32_)
    return (vectorfield, scalarfield, lambda u, t, s, dudt=False: apply_bc_u_(u, t, s, dudt=dudt), lambda F, u, t, s: momentum_(F, u, None, t, s),
            project_)


def _check_precision(single, psolvers, what):
    """A float32 state takes Float32 solvers (`f32.psolver_spectral32` / `f32.psolver_wrap32`), a float64 state fp64 ones: TypeError otherwise."""
    mine, other = ("float32", "float64") if single else ("float64", "float32")
    for ps in psolvers:
        if isinstance(ps, f32.psolver_spectral32) != single:
            raise TypeError(f"{what}: a {mine} state with a {other} pressure solver ({type(ps).__name__}); float32 states take "
                            "f32.psolver_spectral32 / f32.psolver_wrap32 / f32.default_psolver32, float64 states default_psolver and its kin")


def lesdatagen(dnsobs, Φ, les, compression, psolver, dns=None):
    """data_generation.jl:37-60: on every DNS observation `(u, F, t)` store `ū = bc(Φu)` and the commutator error
    `c = ΦF − project(bc(momentum(ū)))` on the host.  The precision is that of the observed `u`: a float32 state runs the chain on the `_f32`
    family and stores float32 arrays."""
    single = _is32(dnsobs.value["u"])
    _check_precision(single, [psolver], "lesdatagen")
    vfield, sfield, bc_u, momentum, project = _ops(single)
    p = sfield(les)
    Φu, FΦ, ΦF = vfield(les), vfield(les), vfield(les)
    results = dict(u=[], c=[])

    def step(obs):
        u, F, t = obs["u"], obs["F"], obs["t"]
        Φ(Φu, u, les, compression, setup_dns=dns)
        bc_u(Φu, t, les)
        Φ(ΦF, F, les, compression, setup_dns=dns)
        momentum(FΦ, Φu, t, les)
        bc_u(FΦ, t, les, dudt=True)
        project(FΦ, les, psolver, p)
        results["u"].append(to_numpy(Φu))
        results["c"].append(to_numpy(ΦF - FΦ))

    dnsobs.on(step)
    return results


def filtersaver(dns, les, filters, compression, psolver_dns, psolver_les, *, nupdate=1, filenames=None, F=None, p=None):
    """Save filtered DNS data (data_generation.jl:62-120): a processor that every `nupdate` steps (and for the initial state) forms
    `F = project(bc(momentum(u)))` on the DNS grid and hands `(u, F, t)` to one `lesdatagen` per (LES grid, filter), LES grid fastest.
    `finalize` returns one dict `(u, c, t, comptime)` per pair, `u` and `c` stacked along a last axis; `filenames` (one per pair) are written
    with `np.savez`.  `F` and `p` are scratch on the DNS grid, allocated here unless given; the processor never writes into the state.
    A float32 state (a Float32 `solve_unsteady`) runs the whole chain in Float32 and stores float32 `u` and `c` (`t` stays double); the solvers are
    then Float32 solvers, and a mix of precisions raises TypeError in `initialize`, before any launch."""
    les, filters, compression, psolver_les = list(les), list(filters), list(compression), list(psolver_les)
    if filenames is not None and len(filenames) != len(les) * len(filters):
        raise ValueError("one file name per (LES grid, filter) pair")
    scratch = dict(F=F, p=p)

    def initialize(state):
        s0 = state.value
        single = _is32(s0["u"])
        _check_precision(single, [psolver_dns] + psolver_les, "filtersaver")
        vfield, sfield, bc_u, momentum, project = _ops(single)
        F = vfield(dns) if scratch["F"] is None else scratch["F"]
        p = sfield(dns) if scratch["p"] is None else scratch["p"]
        if _is32(F) != single or _is32(p) != single:
            raise TypeError(f"filtersaver: the scratch fields F ({F.dtype}) and p ({p.dtype}) must have the precision of the state ({s0['u'].dtype})")
        dnsobs = Observable(dict(u=s0["u"], F=F, t=s0["t"]))
        data = [lesdatagen(dnsobs, Φ, les[i], compression[i], psolver_les[i], dns) for Φ in filters for i in range(len(les))]
        results = dict(data=data, t=[], comptime=time.time())

        def step(s):
            if s["n"] % nupdate != 0:
                return
            u, t = s["u"], s["t"]
            momentum(F, u, t, dns)
            bc_u(F, t, dns, dudt=True)
            project(F, dns, psolver_dns, p)
            results["t"].append(t)
            dnsobs.value = dict(u=u, F=F, t=t)

        state.on(step)
        step(s0)  # save initial conditions
        return results

    def finalize(results, state):
        comptime = time.time() - results["comptime"]
        out = []
        for i, d in enumerate(results["data"]):
            r = dict(u=np.stack(d["u"], axis=-1), c=np.stack(d["c"], axis=-1), t=np.array(results["t"]), comptime=comptime)
            if filenames is not None:
                np.savez(filenames[i], **r)
            out.append(r)
        return out

    return processor(initialize, finalize, nupdate=nupdate)


def create_les_data(*, D, Re, lims, nles, ndns, filters, tburn, tsim, savefreq, Δt=None, method=None, create_psolver=None, icfunc=None,
                    processors=None, rng=None, filenames=None, device=None, dtype=torch.float64, **kwargs):
    """Create filtered DNS data (data_generation.jl:125-223): burn-in DNS from `icfunc(setup, psolver, rng)`, then a DNS of length `tsim` whose
    state is filtered every `savefreq` steps onto every grid of `nles` by every filter.  Returns `filtersaver`'s list.
    `create_psolver` defaults to `default_psolver`.  `dtype=torch.float32` (the reference's `T = Float32`): `create_psolver` defaults to
    `f32.default_psolver32`, the initial field comes from `icfunc` on an fp64 solver, is rounded once and projected with the Float32 solver,
    and burn-in, run, filters and stored arrays are Float32."""
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("create_les_data: dtype is torch.float64 or torch.float32")
    single = dtype == torch.float32
    create_psolver = create_psolver or (f32.default_psolver32 if single else default_psolver)
    method = method or RKMethods.RK44()
    rng = rng if rng is not None else np.random.default_rng()
    nles = list(nles)
    compression = [ndns // n for n in nles]
    if any(c * n != ndns for c, n in zip(compression, nles)):
        raise ValueError("every nles must divide ndns")
    dns = Setup(x=tuple(np.linspace(lims[0], lims[1], ndns + 1) for _ in range(D)), Re=Re, device=device, **kwargs)
    les = [Setup(x=tuple(np.linspace(lims[0], lims[1], n + 1) for _ in range(D)), Re=Re, device=device, **kwargs) for n in nles]
    psolver = create_psolver(dns)
    psolver_les = [create_psolver(s) for s in les]
    if icfunc is None:
        def icfunc(setup, psolver, rng):
            return random_field(setup, 0.0, psolver=psolver, seed=int(rng.integers(2**31 - 1)))
    if single:
        _check_precision(True, [psolver] + psolver_les, "create_les_data(dtype=torch.float32)")
        u = f32.to_f32(dns, icfunc(dns, default_psolver(dns), rng))
        f32.apply_bc_u32_(f32.project32_(f32.apply_bc_u32_(u, dns), dns, psolver, f32.scalarfield32(dns)), dns)
    else:
        u = icfunc(dns, psolver, rng)
    if bool(torch.isnan(u).any()):
        print("Warning: initial conditions contain NaNs")
    processors = dict(processors or {})
    cache = f32.ERKCache32(method, dns, psolver) if single else ode_method_cache(method, dns, psolver)
    if tburn > 0:  # the initial spectrum is artificial: a short simulation makes it realistic
        (u, _, _), _ = solve_unsteady(setup=dns, ustart=u, docopy=False, tlims=(0.0, tburn), Δt=Δt, method=method, psolver=psolver, cache=cache,
                                      processors=processors)
    saver = filtersaver(dns, les, filters, compression, psolver, psolver_les, nupdate=savefreq, filenames=filenames)
    _, outputs = solve_unsteady(setup=dns, ustart=u, docopy=False, tlims=(0.0, tsim), Δt=Δt, method=method, psolver=psolver, cache=cache,
                                processors={**processors, "f": saver})
    return outputs["f"]


_PER_SEED = "call create_les_data once per seed ([create_les_data(…, rng=rng) for _ in range(ntrajectory)])"


def _les_ensemble_refusal(D, Δt, nles, ndns, extra):
    """Why `create_les_data_ensemble` does not take this problem (None: it does).  Host-side facts only: no setup exists yet."""
    if Δt is None:
        return "Δt=None (an adaptive step differs from member to member; the ensemble loop shares one fixed Δt)"
    if D != 2:
        return f"D = {D} (the ensemble loop and the member filters are 2-D)"
    for name, n in [("ndns", ndns)] + [("nles", n) for n in nles]:
        if n != int(n) or n < 16 or n > 1024 or int(n) & (int(n) - 1):
            return f"{name} = {n} (sides must be powers of two in 16 .. 1024: others solve through rocFFT)"
    extra = dict(extra)
    dtype = extra.pop("dtype", torch.float64)
    if dtype != torch.float64:
        return f"dtype = {dtype} (the ensemble loop is fp64)"
    if extra.pop("processors", None):
        return "extra processors (they observe one state; the ensemble has B)"
    if extra.pop("create_psolver", None) is not None:
        return "create_psolver (the ensemble loop runs on psolver_spectral)"
    if extra:
        return f"the Setup keyword(s) {', '.join(sorted(extra))} (the ensemble loop runs the plain all-periodic setup: no body force, closure or other sides)"
    return None


def create_les_data_ensemble(*, ntrajectory, D, Re, lims, nles, ndns, filters, tburn, tsim, savefreq, Δt, method=None, icfunc=None, rng=None, filenames=None,
                             device=None, **kwargs):
    """`[create_les_data(…, rng=rng) for _ in range(ntrajectory)]` with all trajectories advanced and filtered together (2-D periodic, fp64, fixed Δt): one
    `EnsembleCache` on the DNS grid and one per LES grid, the call pattern of `solve_unsteady` with a fixed Δt (burn-in in one `timesteps_ensemble_` call,
    then calls of `savefreq` steps; the initial state is saved first; `t` accumulates as `timesteps_` accumulates it), and at every save one
    `ensemble_rhs_` on the DNS grid and, per (filter, LES grid) pair, LES grid fastest: ONE member-filter launch for `u` and `F` of all members, the member
    ghost fill of ū, `ensemble_rhs_` on the LES cache, one subtraction and one device-to-host copy each of ū and c for the whole ensemble.  The launch count
    per save does not depend on `ntrajectory`.
    The initial fields are `icfunc(dns, psolver, rng)` in member order (default: that of `create_les_data`), so with an identically seeded `rng` member b
    is the b-th of the consecutive `create_les_data` calls: `u` and `t` bitwise, `c` to the rounding of the fused right-hand side.
    Returns a list over members of what `create_les_data` returns (a list of `dict(u, c, t, comptime)` per pair; `comptime` is the whole ensemble's);
    `filenames`: one list per member.  Everything outside the ensemble loop — Δt=None, D=3, a side that is no power of two in 16 .. 1024,
    dtype=torch.float32, processors, any `Setup` keyword — is refused (NotImplementedError) before any launch, naming `create_les_data` per seed."""
    from .setup import vectorfields
    from .time_steppers import LMWray3, EnsembleCache, ensemble_apply_bc_u_, ensemble_rhs_, timesteps_ensemble_

    nles, filters = list(nles), list(filters)
    why = _les_ensemble_refusal(D, Δt, nles, ndns, kwargs)
    if why is not None:
        raise NotImplementedError(f"create_les_data_ensemble: {why} is outside the ensemble route; {_PER_SEED}")
    B = int(ntrajectory)
    if B < 1:
        raise ValueError("an ensemble has at least one member")
    compression = [ndns // n for n in nles]
    if any(c * n != ndns for c, n in zip(compression, nles)):
        raise ValueError("every nles must divide ndns")
    npair = len(nles) * len(filters)
    if filenames is not None and (len(filenames) != B or any(len(f) != npair for f in filenames)):
        raise ValueError("one list of file names per member, each with one name per (LES grid, filter) pair")
    method = method or RKMethods.RK44()
    c_last = 1.0 if isinstance(method, LMWray3) else method.c[-1]  # as timesteps_ advances t
    rng = rng if rng is not None else np.random.default_rng()
    dns = Setup(x=tuple(np.linspace(lims[0], lims[1], ndns + 1) for _ in range(D)), Re=Re, device=device)
    les = [Setup(x=tuple(np.linspace(lims[0], lims[1], n + 1) for _ in range(D)), Re=Re, device=device) for n in nles]
    psolver = default_psolver(dns)
    psolver_les = [default_psolver(s) for s in les]
    if icfunc is None:
        def icfunc(setup, psolver, rng):
            return random_field(setup, 0.0, psolver=psolver, seed=int(rng.integers(2**31 - 1)))
    # the state and its right-hand side share one buffer and one stride, so one filter launch serves both: members 0 .. B-1 are u, B .. 2B-1 are F
    UF = vectorfields(dns, 2 * B)
    U, F = UF[:B], UF[B:]
    for b in range(B):
        U[b].copy_(icfunc(dns, psolver, rng))
    if bool(torch.isnan(U).any()):
        print("Warning: initial conditions contain NaNs")
    try:
        cache = EnsembleCache(method, dns, psolver, B)
        cache_les = [EnsembleCache(method, s, ps, B) for s, ps in zip(les, psolver_les)]
    except NotImplementedError as e:
        raise NotImplementedError(f"create_les_data_ensemble: {e}; {_PER_SEED}") from None
    if tburn > 0:  # solve_unsteady without processors: one native call
        nstep = int(round(tburn / Δt))
        timesteps_ensemble_(cache, U, 0.0, tburn / nstep, nstep)
    VF = [vectorfields(s, 2 * B) for s in les]  # ū = VF[:B], ΦF = VF[B:]
    FΦ = [vectorfields(s, B) for s in les]
    cbuf = [vectorfields(s, B) for s in les]
    pairs = [(Φ, i) for Φ in filters for i in range(len(les))]
    saved = [dict(u=[], c=[]) for _ in pairs]
    ts = []
    comptime = time.time()

    def save(t):
        ensemble_rhs_(cache, F, U)
        for q, (Φ, i) in enumerate(pairs):
            Φ.members(VF[i], UF, les[i], compression[i], setup_dns=dns)
            ū, ΦF = VF[i][:B], VF[i][B:]
            ensemble_apply_bc_u_(cache_les[i], ū)
            ensemble_rhs_(cache_les[i], FΦ[i], ū)
            torch.sub(ΦF, FΦ[i], out=cbuf[i])
            saved[q]["u"].append(ū.cpu().numpy())
            saved[q]["c"].append(cbuf[i].cpu().numpy())
        ts.append(t)

    # solve_unsteady with the saver as its one processor: the steps between the multiples of savefreq run as one native call
    nstep = int(round(tsim / Δt))
    Δt = tsim / nstep
    g = 1 if int(savefreq) <= 1 or os.environ.get("INS_NO_PROCESSOR_BATCH") else int(savefreq)
    t, n, done = 0.0, 0, 0
    save(t)
    while done < nstep:
        k = min(g - (n % g), nstep - done)
        timesteps_ensemble_(cache, U, t, Δt, k)
        t = t + k * c_last * Δt if k > 1 else t + c_last * Δt
        n += k
        done += k
        if n % savefreq == 0:
            save(t)
    comptime = time.time() - comptime
    out = []
    for b in range(B):
        member = []
        for q in range(len(pairs)):
            r = dict(u=np.stack([np.asfortranarray(a[b]) for a in saved[q]["u"]], axis=-1),
                     c=np.stack([np.asfortranarray(a[b]) for a in saved[q]["c"]], axis=-1), t=np.array(ts), comptime=comptime)
            if filenames is not None:
                np.savez(filenames[b][q], **r)
            member.append(r)
        out.append(member)
    return out


def create_io_arrays(data, setup):
    """Create (ū, c) pairs for a-priori training (data_generation.jl:228-252): `data` is a list of trajectories `dict(u, c, t)` on the grid of
    `setup`; returns `dict(u, c)` of numpy arrays `(n…, D, nsample)` holding `Iu[α]` of every component, trajectories joined along the
    sample axis.  The arrays have the dtype of the data: float32 trajectories give float32 arrays."""
    g = setup.grid
    D = g.dimension
    out = {}
    for key in ("u", "c"):
        parts = []
        for traj in data:
            nt = len(traj["t"])
            src = np.asarray(traj[key])
            a = np.zeros(tuple(n - 2 for n in g.N) + (D, nt), dtype=src.dtype if src.dtype == np.float32 else np.float64)
            for α in range(D):
                sl = tuple(slice(lo, hi) for lo, hi in g.Iu[α])
                a[..., α, :] = src[sl + (α, slice(None))]
            parts.append(a)
        out[key] = np.concatenate(parts, axis=-1)
    return out


# ------------------------------------------------------------------------------------------------ closure.jl, cnn.jl
def _inside(setup):
    Iu = setup.grid.Iu
    if any(I != Iu[0] for I in Iu):
        raise ValueError("Only periodic grids are supported")
    return tuple(slice(lo, hi) for lo, hi in Iu[0])


def wrappedclosure(m, setup):
    """Wrap closure model `m(x, θ)` on `(n…, D, nsample)` arrays so that it can be used in the solver (closure.jl:4-17): the interior of the
    padded field goes in as one sample, the result is padded periodically (ghosts = the opposite interior layer).  Differentiable."""
    inside = _inside(setup)
    D = setup.grid.dimension

    def neuralclosure(u, θ):
        mu = m(u[inside].unsqueeze(-1), θ).squeeze(-1)
        for d in range(D):
            mu = torch.cat([mu.narrow(d, mu.shape[d] - 1, 1), mu, mu.narrow(d, 0, 1)], dim=d)
        return mu

    return neuralclosure


def wrappedclosure_ensemble(m, setup):
    """`wrappedclosure` for the B members of an ensemble field `(B,) + N + (2,)` (`vectorfields`): the interiors of all members go into `m` as B samples,
    `(n0, n1, 2, B)`, in ONE call, the result is padded periodically and comes back in the layout of `vectorfields`.  Differentiable; no loop over B.
    A member closure for `ad.timestep_ensemble` and `create_loss_post_ensemble`."""
    inside = _inside(setup)
    if setup.grid.dimension != 2:
        raise NotImplementedError("wrappedclosure_ensemble: a 3-D setup is outside the member operators (2-D); wrap the model with wrappedclosure and use "
                                  "ad.timestep / create_loss_post per trajectory")

    def neuralclosure_ensemble(U, θ):
        x = U[(slice(None),) + inside].permute(1, 2, 3, 0)  # (n0, n1, 2, B)
        mu = m(x, θ).permute(3, 2, 1, 0)  # (B, 2, n1, n0): the memory order of `vectorfields`
        for d in (2, 3):
            mu = torch.cat([mu.narrow(d, mu.shape[d] - 1, 1), mu, mu.narrow(d, 0, 1)], dim=d)
        return mu.permute(0, 3, 2, 1)

    return neuralclosure_ensemble


def collocate(u):
    """Interpolate velocity components to volume centers (closure.jl:37-72): `(n…, D, nsample)`, out[i] = (u_α[i] + u_α[i − e_α]) / 2,
    periodic."""
    D = u.shape[-2]
    return torch.stack([(u[..., a, :] + torch.roll(u[..., a, :], 1, dims=a)) / 2 for a in range(D)], dim=-2)


def decollocate(u):
    """Interpolate closure force from volume centers to volume faces (closure.jl:74-108): out[i] = (u_α[i] + u_α[i + e_α]) / 2, periodic."""
    D = u.shape[-2]
    return torch.stack([(u[..., a, :] + torch.roll(u[..., a, :], -1, dims=a)) / 2 for a in range(D)], dim=-2)


class _ConvFoldedSamples(torch.autograd.Function):
    """`conv2d(x, w, b)` of the ONE sample that `CNN(batched=True)` folds all samples into, with the weight gradient summed in chunks.  torch's own float64
    weight gradient is one GEMM with an 8 x 50-sized result and the whole folded plane as its inner dimension; the library kernel chosen for it runs that
    reduction in a single workgroup and was measured at 3.5 ms per call for 18 000 columns (88 % of a loss evaluation at 32², B = 16).  Here the columns are
    cut into chunks of `CHUNK`, one batched GEMM forms the partial sums side by side and one sum adds them: two launches whatever the plane's size."""

    CHUNK = 2048

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return torch.nn.functional.conv2d(x, w, b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx = torch.nn.grad.conv2d_input(x.shape, w, g) if ctx.needs_input_grad[0] else None
        gw = gb = None
        G = g.reshape(g.shape[1], -1)  # (Cout, N): one sample
        if ctx.needs_input_grad[1]:
            cols = torch.nn.functional.unfold(x, w.shape[2:])[0]  # (Cin·k², N)
            n = _ConvFoldedSamples.CHUNK
            S = -(-G.shape[1] // n)
            pad = S * n - G.shape[1]
            Gp, cp = torch.nn.functional.pad(G, (0, pad)), torch.nn.functional.pad(cols, (0, pad))
            parts = torch.bmm(Gp.reshape(G.shape[0], S, n).transpose(0, 1), cp.reshape(cols.shape[0], S, n).permute(1, 2, 0))  # (S, Cout, Cin·k²)
            gw = parts.sum(0).reshape(w.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = G.sum(1)
        return gx, gw, gb


class CNN(torch.nn.Module):
    """collocate → circular padding by Σ radii → convolutions (kernel 2r+1, no further padding) → decollocate (cnn.jl); float64 parameters, or
    float32 with `dtype=torch.float32`.

    `batched=True` (off by default): the convolutions see all samples as ONE sample.  torch convolves float64 tensors sample by sample (im2col, GEMM,
    col2im per sample), so the launch count of a forward and backward grows with the number of samples.  The convolutions take no padding of their own,
    so the circularly padded samples can be laid side by side along the first spatial axis: an output row of sample b reads rows of sample b's own padded
    block only, the rows that straddle two samples are computed and dropped (2·Σradii of every n + 2·Σradii rows).  Same sums per output value in another
    GEMM blocking: the result agrees with `batched=False` to rounding, and the launch count does not depend on the number of samples.  In 2-D the weight
    gradient of the folded sample is summed in chunks (`_ConvFoldedSamples`)."""

    def __init__(self, D, radii, channels, activations, use_bias, generator=None, dtype=torch.float64, batched=False):
        super().__init__()
        self.batched = bool(batched)
        if dtype not in (torch.float64, torch.float32):
            raise TypeError("cnn: dtype is torch.float64 or torch.float32")
        if channels[-1] != D:
            raise ValueError("the last layer must have D channels (one force field per direction)")
        self.D, self.pad, self.activations = D, int(sum(radii)), list(activations)
        c = [D] + list(channels)
        Conv = torch.nn.Conv2d if D == 2 else torch.nn.Conv3d
        self.convs = torch.nn.ModuleList(Conv(c[i], c[i + 1], 2 * radii[i] + 1, bias=bool(use_bias[i]), dtype=dtype) for i in range(len(radii)))
        for conv in self.convs:  # glorot_uniform weights, zero bias, as Lux's Conv with init_weight = glorot_uniform
            torch.nn.init.xavier_uniform_(conv.weight, generator=generator)
            if conv.bias is not None:
                torch.nn.init.zeros_(conv.bias)

    def forward(self, u, θ=None):
        if θ is not None:
            return torch.func.functional_call(self, θ, (u,))
        D = self.D
        x = collocate(u)
        x = x.permute(D + 1, D, *range(D))  # (nsample, D, n…)
        x = torch.nn.functional.pad(x, (self.pad,) * (2 * D), mode="circular")
        nsample, n0, rows = x.shape[0], x.shape[2] - 2 * self.pad, x.shape[2]
        if self.batched:  # (nsample, C, Hp, …) -> (1, C, nsample·Hp, …)
            x = x.transpose(0, 1).reshape(1, x.shape[1], nsample * rows, *x.shape[3:])
        for conv, σ in zip(self.convs, self.activations):
            x = _ConvFoldedSamples.apply(x, conv.weight, conv.bias) if self.batched and D == 2 else conv(x)
            if σ is not None:
                x = σ(x)
        if self.batched:  # rows b·Hp … b·Hp + n0 − 1 are sample b's; the 2·pad rows the convolutions consumed are put back so that the blocks line up
            x = torch.nn.functional.pad(x, (0, 0) * (D - 1) + (0, 2 * self.pad))
            x = x.reshape(x.shape[1], nsample, rows, *x.shape[3:]).narrow(2, 0, n0).transpose(0, 1)
        x = x.permute(*range(2, D + 2), 1, 0)
        return decollocate(x)


def cnn(*, setup, radii, channels, activations, use_bias, rng=None, dtype=torch.float64, batched=False):
    """Create CNN closure model (cnn.jl): a `torch.nn.Module` on the device of `setup`, callable as `m(x, θ)`.  `activations[i]` is a
    callable or None (identity); `rng`: a `torch.Generator` (CPU) or an integer seed for the weights; `dtype`: the precision of the
    parameters, and so of the arrays the model takes (torch.float64 or torch.float32).  `batched=True`: all samples of a call go through the
    convolutions as one (see `CNN`), for member closures (`wrappedclosure_ensemble`); same parameters and, to rounding, the same result."""
    gen = rng
    if rng is not None and not isinstance(rng, torch.Generator):
        gen = torch.Generator().manual_seed(int(rng))
    return CNN(setup.grid.dimension, list(radii), list(channels), activations, use_bias, gen, dtype, batched).to(setup.device)


class TensorClosure(torch.nn.Module):
    """Tensor-basis closure of Silvis et al. (tensorbasis.jl): c = divoftensor(bc_p(Σ_i a_i(V) B_i)) with the coefficients a pointwise network of
    the invariants — linear layers over the channel axis, float64 (or float32: then the operators are those of `ins_amd.ad32`, on float32
    fields).  Frame-invariant by construction, and defined on every grid the kernels of csrc/ins_tensorclosure.hip (ins_tensorclosure32.hip)
    accept.  Called on the padded field: `m(u, θ)`."""

    def __init__(self, setup, hidden, activation, generator=None, dtype=torch.float64):
        super().__init__()
        from .operators import _tb_sizes

        if dtype not in (torch.float64, torch.float32):
            raise TypeError("tensorclosure: dtype is torch.float64 or torch.float32")
        self.setup, self.activation = setup, activation
        self.dtype = dtype
        nb, nv, _ = _tb_sizes(setup)
        c = [nv] + list(hidden) + [nb]
        self.layers = torch.nn.ModuleList(torch.nn.Linear(c[i], c[i + 1], dtype=dtype) for i in range(len(c) - 1))
        for layer in self.layers:  # glorot_uniform weights, zero bias, as `cnn`
            torch.nn.init.xavier_uniform_(layer.weight, generator=generator)
            torch.nn.init.zeros_(layer.bias)

    def coefficients(self, V):
        """a = MLP(V) per cell: N + (nv,) -> N + (nb,)."""
        x = V
        for i, layer in enumerate(self.layers):
            x = layer(x)
            if i + 1 < len(self.layers) and self.activation is not None:
                x = self.activation(x)
        return x

    def forward(self, u, θ=None):
        if θ is not None:
            return torch.func.functional_call(self, θ, (u,))
        from . import autodiff32

        s, o = self.setup, (ad if self.dtype == torch.float64 else autodiff32)
        a = self.coefficients(o.tensorinvariants(u, s))
        τ = o.apply_bc_p_fields(o.tensorclosure_stress(u, a, s), 0.0, s)
        return o.divoftensor(τ, s)


def tensorclosure(*, setup, hidden, activation, rng=None, dtype=torch.float64):
    """Create tensor-basis closure model: a float64 `torch.nn.Module` on the device of `setup`, callable as `m(u, θ)` on the padded field, so it
    is a `closure_model` for `create_loss_post`, `create_relerr_post` and `ad.timestep` as it stands.  `hidden`: widths of the hidden layers of
    the coefficient network V -> a; `activation`: a callable or None; `rng`: a `torch.Generator` (CPU) or an integer seed for the weights;
    θ = None uses the module's own parameters, a dict goes through `torch.func.functional_call`.  The invariants enter as they are: scale them
    in `activation` / the first layer if the flow needs it.  `dtype=torch.float32`: float32 layers on the `ad32` operators, a `closure_model`
    for `ad32.timestep` and for `create_loss_post` with a Float32 pressure solver."""
    gen = rng
    if rng is not None and not isinstance(rng, torch.Generator):
        gen = torch.Generator().manual_seed(int(rng))
    return TensorClosure(setup, list(hidden), activation, gen, dtype).to(setup.device)


# ------------------------------------------------------------------------------------------------ training.jl
def _as_tensor(a, device, dtype=None):
    """`a` on `device`; `dtype=None`: float64."""
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a, dtype=dtype or torch.float64, device=device)


def create_dataloader_prior(data, *, batchsize=50, device=None, dtype=None):
    """training.jl:1-23: `dataloader(rng) -> ((x, y), rng)`, a batch of `batchsize` random samples (sorted indices) on `device`.
    `rng` is a `numpy.random.Generator`.  `dtype`: the precision of the batches (None: float64)."""
    x, y = data
    nsample = x.shape[-1]

    def dataloader(rng):
        i = np.sort(rng.permutation(nsample)[:batchsize])
        return (_as_tensor(x[..., i], device, dtype), _as_tensor(y[..., i], device, dtype)), rng

    return dataloader


def create_dataloader_post(trajectories, *, ntrajectory, nunroll, device=None, dtype=None):
    """Create trajectory dataloader (training.jl:25-41): `ntrajectory` random trajectories, of each `nunroll + 1` consecutive states from a
    random start.  `dtype`: the precision of the states (None: float64); `t` stays a double array."""

    def dataloader(rng):
        data = []
        for k in rng.permutation(len(trajectories))[:ntrajectory]:
            u, t = trajectories[k]["u"], np.asarray(trajectories[k]["t"])
            nt = len(t)
            if nt < nunroll + 1:
                raise ValueError(f"Trajectory too short for nunroll = {nunroll}")
            istart = int(rng.integers(0, nt - nunroll))
            it = slice(istart, istart + nunroll + 1)
            data.append(dict(u=_as_tensor(u[..., it], device, dtype), t=t[it]))
        return data, rng

    return dataloader


def train(*, dataloader, loss, trainstate, niter, callback=None, callbackstate=None, λ=None):
    """training.jl:43-63: `niter` times: batch, gradient of `loss(batch, θ)`, optional weight decay `g += λθ`, optimiser step, callback.
    `trainstate = dict(opt=<torch.optim optimiser over the parameters>, θ=<what the loss takes>, rng=<numpy Generator>)`."""
    opt, θ, rng = trainstate["opt"], trainstate["θ"], trainstate["rng"]
    for _ in range(niter):
        batch, rng = dataloader(rng)
        opt.zero_grad(set_to_none=True)
        loss(batch, θ).backward()
        if λ is not None:
            for group in opt.param_groups:
                for q in group["params"]:
                    if q.grad is not None:
                        q.grad.add_(q.detach(), alpha=λ)
        opt.step()
        trainstate = dict(opt=opt, θ=θ, rng=rng)
        if callback is not None:
            callbackstate = callback(callbackstate, trainstate)
    return dict(trainstate=trainstate, callbackstate=callbackstate)


def create_loss_prior(f, normalize=None):
    """Return mean squared error loss for the predictor `f` (training.jl:110-113): Σ(f(x, θ) − y)² / normalize(y), default Σy²."""
    normalize = normalize or (lambda y: (y * y).sum())

    def loss_prior(batch, θ):
        x, y = batch
        d = f(x, θ) - y
        return (d * d).sum() / normalize(y)

    return loss_prior


def create_relerr_prior(f, x, y):
    """Create a-priori error (training.jl:115-118): θ -> ‖f(x, θ) − y‖ / ‖y‖."""

    def relerr_prior(θ):
        with torch.no_grad():
            return float(torch.linalg.vector_norm(f(x, θ) - y) / torch.linalg.vector_norm(y))

    return relerr_prior


class _SetupView(Setup):
    """`(; setup..., closure_model)`: the same grid handle and device, another closure model.  Keeps its parent alive; owns nothing."""

    def __init__(self, parent, closure_model):
        self.__dict__.update(parent.__dict__)
        self._parent, self.closure_model = parent, closure_model

    def __del__(self):
        pass


def _field_of(setup, a):
    f = vectorfield(setup)
    f.copy_(a)
    return f


def create_loss_post(*, setup, method, psolver, closure_model, nsubstep=1):
    """Create a-posteriori loss function (training.jl:120-146): unroll `ad.timestep` from the first state of every trajectory in the batch and
    average Σ|u − u_ref|² / Σ|u_ref|² (on `Iu`) over the following states.  Differentiable in θ.  With a Float32 pressure solver
    (`f32.psolver_spectral32`, `f32.psolver_wrap32`) the step is `ad32.timestep` on float32 fields (the trajectories are rounded to float32)."""
    from . import autodiff32

    setup = _SetupView(setup, closure_model)
    inside = _inside(setup)
    single = isinstance(psolver, f32.psolver_spectral32)
    step = autodiff32.timestep if single else ad.timestep

    def loss_post(data, θ):
        total = 0.0
        for traj in data:
            u, t = traj["u"], traj["t"]
            if single:
                u = u.float()
            u0 = f32.to_f32(setup, u[..., 0]) if single else _field_of(setup, u[..., 0])
            stepper = create_stepper(method, setup=setup, psolver=psolver, u=u0, temp=None, t=float(t[0]))
            loss = 0.0
            for it in range(1, len(t)):
                Δt = float(t[it] - t[it - 1]) / nsubstep
                for _ in range(nsubstep):
                    stepper = step(method, stepper, Δt, θ)
                uref = u[..., it][inside]
                d = stepper.u[inside] - uref
                loss = loss + (d * d).sum() / (uref * uref).sum()
            total = total + loss / (len(t) - 1)
        return total / len(data)

    return loss_post


def _post_ensemble_steps(data):
    """The shared step sizes `t[it] − t[it−1]` of a batch of trajectories (start times may differ: nothing depends on t).  ValueError for trajectories of
    different lengths or step sizes.  Two saved times carry a rounding error of eps·|t| each, so their difference is known to 2·eps·max|t|, and two such
    differences compare to 4·eps·max|t| (absolute): sizes that agree within that are the same step, and the first trajectory's are used."""
    ts = [np.asarray(traj["t"], dtype=np.float64) for traj in data]
    if not ts:
        raise ValueError("create_loss_post_ensemble: an empty batch")
    dts = np.diff(ts[0])
    for t in ts[1:]:
        if len(t) != len(ts[0]):
            raise ValueError(f"create_loss_post_ensemble: trajectories of {len(ts[0])} and {len(t)} states in one batch; the ensemble step advances all "
                             f"members together; {_PER_TRAJECTORY}")
        tol = 4 * np.finfo(np.float64).eps * max(np.abs(t).max(), np.abs(ts[0]).max())
        if not np.all(np.abs(np.diff(t) - dts) <= tol):
            raise ValueError(f"create_loss_post_ensemble: the trajectories of the batch have different step sizes (the ensemble step shares one Δt); "
                             f"{_PER_TRAJECTORY}")
    return dts


def create_loss_post_ensemble(*, setup, method, psolver, closure_model, nsubstep=1):
    """`create_loss_post` with all trajectories of the batch in ONE unrolled graph (`ad.timestep_ensemble`): the B first states go into one ensemble
    field, every step advances all members, and the same per-trajectory normalised error sums Σ|u − u_ref|² / Σ|u_ref|² (on `Iu`) are averaged over
    trajectories and states.  The launch count of the step's operators and of their backward does not depend on B; the closure's is its own (torch convolves
    float64 tensors sample by sample: a `cnn(..., batched=True)` keeps the whole evaluation independent of B).  `data`: the batch format of
    `create_dataloader_post`; all trajectories share `len(t)` and the step sizes (ValueError otherwise, naming `create_loss_post`).  `closure_model`: a
    member closure (`wrappedclosure_ensemble(m, setup)`) or None.  One `EnsembleCache` per B is built on first use and kept.

    Scope: that of `EnsembleCache` (fp64, 2-D, all-periodic, uniform, power-of-two sides 16 … 1024, `psolver_spectral`, a method with more than one stage, no
    body force / temperature / closure on the setup itself); everything else raises NotImplementedError naming `create_loss_post`."""
    from .time_steppers import EnsembleCache, LMWray3, _ensemble_refusal, _lmwray3_as_erk
    from .setup import vectorfields

    erk = _lmwray3_as_erk(method) if isinstance(method, LMWray3) else method
    why = "a Float32 pressure solver (the member operators are fp64)" if isinstance(psolver, f32.psolver_spectral32) else _ensemble_refusal(erk, setup, psolver)
    if why is not None:
        raise NotImplementedError(f"create_loss_post_ensemble: {why} is outside the ensemble route; {_PER_TRAJECTORY}")
    nsubstep = int(nsubstep)
    if nsubstep < 1:
        raise ValueError("nsubstep must be at least 1")
    inside = (slice(None),) + _inside(setup)
    caches = {}

    def loss_post_ensemble(data, θ):
        dts = _post_ensemble_steps(data)
        B = len(data)
        if B not in caches:
            try:
                caches[B] = EnsembleCache(erk, setup, psolver, B)
            except NotImplementedError as e:  # the library's own predicate: a grid that is not exactly uniform, a run-time switch
                raise NotImplementedError(f"create_loss_post_ensemble: {e}; {_PER_TRAJECTORY}") from None
        cache = caches[B]
        ref = torch.stack([traj["u"] for traj in data]).to(dtype=torch.float64, device=setup.device)  # (B,) + N + (2, nt)
        U = vectorfields(setup, B)
        U.copy_(ref[..., 0])
        loss = 0.0
        for it in range(1, len(dts) + 1):
            Δt = float(dts[it - 1]) / nsubstep
            for _ in range(nsubstep):
                U = ad.timestep_ensemble(erk, cache, U, 0.0, Δt, θ, closure_model)
            uref = ref[..., it][inside]
            d = U[inside] - uref
            loss = loss + ((d * d).sum(dim=(1, 2, 3)) / (uref * uref).sum(dim=(1, 2, 3))).sum()
        return loss / (len(dts) * B)

    return loss_post_ensemble


def create_relerr_post(*, data, setup, method, psolver, closure_model, nsubstep=1):
    """Create a-posteriori relative error (training.jl:148-180): θ -> mean over the trajectory of ‖u − u_ref‖ / ‖u_ref‖ (on `Iu`), the LES run
    with the native mutating `timestep_`.  With a Float32 pressure solver the fields are float32 and the step is `ad32.timestep` under
    `torch.no_grad()`: the native Float32 stage loop runs the library's Smagorinsky closure only, not a torch closure."""
    from . import autodiff32

    setup = _SetupView(setup, closure_model)
    inside = _inside(setup)
    single = isinstance(psolver, f32.psolver_spectral32)
    u, t = _as_tensor(data["u"], setup.device, torch.float32 if single else None), np.asarray(data["t"])
    if single:
        def relerr_post32(θ):
            with torch.no_grad():
                stepper = create_stepper(method, setup=setup, psolver=psolver, u=f32.to_f32(setup, u[..., 0]), temp=None, t=float(t[0]))
                e = 0.0
                for it in range(1, len(t)):
                    Δt = float(t[it] - t[it - 1]) / nsubstep
                    for _ in range(nsubstep):
                        stepper = autodiff32.timestep(method, stepper, Δt, θ)
                    uref = u[..., it][inside]
                    e += float(torch.linalg.vector_norm(stepper.u[inside] - uref) / torch.linalg.vector_norm(uref))
                return e / (len(t) - 1)

        return relerr_post32
    v = vectorfield(setup)
    cache = ode_method_cache(method, setup, psolver)

    def relerr_post(θ):
        with torch.no_grad():
            v.copy_(u[..., 0])
            stepper = create_stepper(method, setup=setup, psolver=psolver, u=v, temp=None, t=float(t[0]))
            e = 0.0
            for it in range(1, len(t)):
                Δt = float(t[it] - t[it - 1]) / nsubstep
                for _ in range(nsubstep):
                    stepper = timestep_(method, stepper, Δt, θ=θ, cache=cache)
                uref = u[..., it][inside]
                e += float(torch.linalg.vector_norm(stepper.u[inside] - uref) / torch.linalg.vector_norm(uref))
            return e / (len(t) - 1)

    return relerr_post
