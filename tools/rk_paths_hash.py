#!/usr/bin/env python3
"""One SHA-256 per stage-loop path of the Runge-Kutta drivers (csrc/ins_rk.hip, ins_rk_ext.hip, ins_f32.hip): u (and temp, p where they exist) after a few
steps from a fixed seeded field, with the route counters (stage kernels that wrote the Poisson right-hand side, graph replays, fused ext steps) beside it.
The Float32 family adds one line per solver route (projection, solver call, divergence maximum), extended-loop case and `ad32.timesteps` gradient.
For a change that must not move a bit: run it on both builds (INS_HIP_LIB selects the library) on the same machine and diff the two outputs.

    python tools/rk_paths_hash.py [--only REGEX] > hashes.txt

Every case is the smallest box its path accepts (the shapes of tests/test_gpu_parity.py, test_gpu_fields.py, test_gpu_f32.py)."""
import argparse
import ctypes as C
import hashlib
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ins_amd as ins  # noqa: E402
from ins_amd import _lib  # noqa: E402

DT = 2e-3  # or half the CFL step of the start field where that is smaller (the stretched wall-bounded grids)
NONFINITE = []
VARIANTS = (("", {}), ("keepk", dict(INS_RK_KEEP_K=1)), ("nocorr", dict(INS_DISABLE_INKERNEL_CORR=1)))


def randn(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).standard_normal(shape))


def cosine(a, b, n):
    return a + (b - a) * (1 - np.cos(np.pi * np.arange(n + 1) / n)) / 2


def tanh(a, b, n, g):
    return a + (b - a) * (1 + np.tanh(g * (2 * np.linspace(0.0, 1.0, n + 1) - 1)) / np.tanh(g)) / 2


def exact(n):
    """uniform spacings that are exact binary fractions (the in-kernel correction needs them)"""
    return tuple(np.arange(ni + 1) / 2.0 ** int(np.ceil(np.log2(ni))) for ni in n)


def force(a, x, y, *zt):
    return (a == 0) * (1.0 + np.sin(2 * np.pi * y)) + (a == 1) * 0.3 * np.cos(2 * np.pi * x) + 0 * sum(zt[:-1], 0.0)


P, Dn = ins.PeriodicBC, ins.DirichletBC
LID = (1.0, 0.2, 0.0)


def moving_lid(al, x, y, z, t):
    return (al == 0) * (1.0 + 0.5 * np.sin(3.0 * t)) * np.sin(np.pi * x) ** 2 + (al == 2) * 0.2 * np.cos(2.0 * t) + 0 * (x + y + z)


def geometry(name):
    """(x, boundary conditions or None, pressure solver constructor)"""
    if name.startswith("per"):  # per32x32x32, per64x32
        return exact(tuple(int(v) for v in name[3:].split("x"))), None, ins.psolver_spectral
    kind, nx = name.rstrip("0123456789"), int(re.search(r"\d+$", name).group())
    if kind == "cavity":
        return (cosine(0.0, 1.0, nx), cosine(0.0, 1.0, 48), np.linspace(-0.2, 0.2, 33)), ((Dn(), Dn()), (Dn(), Dn(LID)), (P(), P())), ins.psolver_direct
    if kind == "channel":
        return (np.linspace(0.0, 2.0, nx + 1), tanh(0.0, 1.0, 48, 1.5), np.linspace(0.0, 1.0, 33)), ((P(), P()), (Dn(), Dn()), (P(), P())), ins.psolver_direct
    if kind == "walls":  # small wall-bounded 3-D box
        return (tanh(0.0, 1.0, nx, 1.2), cosine(0.0, 1.0, 10), np.linspace(-0.2, 0.2, 9)), ((Dn(), Dn()), (Dn(), Dn(LID)), (P(), P())), ins.psolver_direct
    if kind == "dirichlet2d":
        return (cosine(0.0, 1.0, nx), tanh(0.0, 1.0, 10, 1.2)), ((Dn(), Dn()), (Dn(), Dn((1.0, 0.0)))), ins.psolver_direct
    if kind == "lidbc":  # time-dependent wall data: ins_rk_step_bc_f64
        return (cosine(0.0, 1.0, nx), cosine(0.0, 1.0, 10), np.linspace(-0.2, 0.2, 9)), ((Dn(), Dn()), (Dn(), Dn(moving_lid)), (P(), P())), ins.psolver_direct
    raise ValueError(name)


def sha(label, *fields):
    """a field that has blown up would hash the same whatever the coefficients were: such a case is reported, not hashed"""
    h = hashlib.sha256()
    for f in fields:
        if not np.all(np.isfinite(f)):
            NONFINITE.append(label)
            return "NONFINITE".ljust(64)
        h.update(np.ascontiguousarray(f).tobytes())
    return h.hexdigest()


def pressure(cache, sp):
    import torch

    ptr = C.c_void_p()
    _lib.call("ins_rk_pressure", cache.handle, C.byref(ptr))
    torch.cuda.synchronize()
    out = np.empty(int(np.prod(sp.grid.N)), dtype=np.float64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def counters(cache):
    lib = _lib.load()
    k = C.c_int64()
    _lib.call("ins_dbg_stage_rhs_used", cache.handle, C.byref(k))
    lib.ins_dbg_rk_graph_replays.restype, lib.ins_dbg_rk_graph_replays.argtypes = C.c_longlong, [C.c_void_p]
    lib.ins_dbg_ext_fused_steps.restype = C.c_longlong
    return k.value, int(lib.ins_dbg_rk_graph_replays(cache.handle)), int(lib.ins_dbg_ext_fused_steps())


class Setups:
    """one Setup, solver and start field per (geometry, force, temperature, closure)"""

    def __init__(self):
        self.made = {}

    def get(self, geom, with_force=False, temp=False, smag=False, user=False):
        key = (geom, with_force, temp, smag, user)
        if key not in self.made:
            x, bc, mk = geometry(geom)
            kw = {}
            if bc is not None:
                kw["boundary_conditions"] = bc
            if with_force:
                kw.update(bodyforce=force, issteadybodyforce=True)
            if temp:
                per = (P(), P())
                kw["temperature"] = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per,) * len(x), gdir=1, dodissipation=True)
            else:
                kw["Re"] = 200.0
            sp = ins.Setup(x=x, **kw)
            if smag:
                sp.closure_model = ins.smagorinsky_closure(sp)
            if user:  # a callable the library knows nothing about: only the host stage loop can evaluate it
                sp.closure_model = lambda u, θ: θ * u
            ps = mk(sp)
            D = len(x)
            u0 = ins.apply_bc_u(ins.project(ins.apply_bc_u(ins.from_numpy(sp, 0.1 * randn(sp.grid.N + (D,), 11)), 0.0, sp), sp, ps), 0.0, sp)
            t0 = ins.apply_bc_temp(ins.from_numpy(sp, 0.5 + 0.1 * randn(sp.grid.N, 4)), 0.0, sp) if temp else None
            self.made[key] = (sp, ps, u0, t0, min(DT, 0.5 * ins.get_cfl_timestep_(None, u0, sp)))
        return self.made[key]


def run_f64(S, label, geom, method, mode, opts, with_force=False, temp=False, smag=False, user=False, host_loop=False):
    sp, ps, u0, t0, dt = S.get(geom, with_force, temp, smag, user)
    m = ins.LMWray3() if method == "LMWray3" else getattr(ins.RKMethods, method)()
    theta = 0.17 if smag or user else None
    before = int(_lib.load().ins_dbg_ext_fused_steps())
    if host_loop:
        os.environ["INS_HOST_STAGE_LOOP"] = "1"
    try:
        with _lib.options(**opts):
            cache = ins.ode_method_cache(m, sp, ps)
            st = ins.create_stepper(m, setup=sp, psolver=ps, u=u0.clone(), temp=None if t0 is None else t0.clone())
            if mode == "single":
                for _ in range(3):
                    st = ins.timestep_(m, st, dt, θ=theta, cache=cache)
            else:  # chainN / graphN: one native call of N steps
                st = ins.timesteps_(m, st, dt, int(mode[5:]), θ=theta, cache=cache)
            # the pressure of the loop that ran: the host loops keep theirs in a field of the cache, the native ones in the handle
            if method == "LMWray3":
                rk, hostp = (cache._erk[1] if cache._erk else None), (cache.p if cache._host else None)
            else:
                rk, hostp = cache, (cache._host["p"] if hasattr(cache, "_host") else None)
            fields = [ins.to_numpy(st.u)] + ([ins.to_numpy(st.temp)] if st.temp is not None else [])
            fields.append(ins.to_numpy(hostp) if hostp is not None else pressure(rk, sp))
            rhs, replays, fused = counters(rk) if rk is not None else (0, 0, before)
    finally:
        os.environ.pop("INS_HOST_STAGE_LOOP", None)
    print(f"{label:58s} {sha(label, *fields)} rhs={rhs} replays={replays} extfused={fused - before}", flush=True)


def run_f32(label, x, bc, method, nsteps, chained, opts):
    f32 = ins.f32
    sp = ins.Setup(x=x, Re=500.0, **({} if bc is None else {"boundary_conditions": bc}))
    D = len(x)
    ps64 = ins.default_psolver(sp)
    u0 = ins.apply_bc_u(ins.project(ins.apply_bc_u(ins.from_numpy(sp, 0.1 * randn(sp.grid.N + (D,), 5)), 0.0, sp), sp, ps64), 0.0, sp)
    dt = min(DT, 0.5 * ins.get_cfl_timestep_(None, u0, sp))
    with _lib.options(**opts):
        ps = f32.default_psolver32(sp)
        cache = f32.ERKCache32(getattr(ins.RKMethods, method)(), sp, ps)
        u = f32.to_f32(sp, ins.to_numpy(u0))
        if chained:
            f32.timesteps32_(cache, u, dt, nsteps)
        else:
            for _ in range(nsteps):
                f32.timestep32_(cache, u, dt)
        print(f"{label:58s} {sha(label, u.cpu().numpy())}", flush=True)
    del cache, ps


def setup32(geom, with_force=False, temp=False, smag=False, wrap=None):
    """Setup, Float32 solver and projected float32 start field(s) of a Float32 case.  wrap: None (default_psolver32), or the constructor of the fp64
    solver psolver_wrap32 goes around."""
    f32 = ins.f32
    x, bc, _ = geometry(geom)
    D = len(x)
    kw = {} if bc is None else {"boundary_conditions": bc}
    if with_force:
        kw.update(bodyforce=force, issteadybodyforce=True)
    if temp:
        tbcs = ((P(), P()),) * D if bc is None else ((ins.SymmetricBC(), ins.SymmetricBC()), (Dn(1.0), Dn(0.0)), (P(), P()))
        kw["temperature"] = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=tbcs, gdir=1, dodissipation=True)
    else:
        kw["Re"] = 500.0
    sp = ins.Setup(x=x, **kw)
    if smag:
        sp.closure_model = f32.smagorinsky_closure32(sp)
    u0 = ins.apply_bc_u(ins.project(ins.apply_bc_u(ins.from_numpy(sp, 0.1 * randn(sp.grid.N + (D,), 5)), 0.0, sp), sp, ins.default_psolver(sp)), 0.0, sp)
    dt = min(DT, 0.5 * ins.get_cfl_timestep_(None, u0, sp))
    t0 = f32.apply_bc_temp32_(f32.to_f32(sp, 0.5 + 0.1 * randn(sp.grid.N, 4)), sp) if temp else None
    return sp, (lambda: f32.default_psolver32(sp) if wrap is None else f32.psolver_wrap32(sp, wrap(sp))), f32.to_f32(sp, ins.to_numpy(u0)), t0, dt


def run_f32_solver(label, geom, pre, post, wrap=None):
    """project32_ (u and p), the solver call on a padded p and max_abs_divergence32, one hash each; `pre` is set before the solver is created, `post` after"""
    f32 = ins.f32
    sp, mkps, u0, _, _ = setup32(geom, wrap=wrap)
    raw = f32.to_f32(sp, 0.1 * randn(sp.grid.N + (len(sp.grid.N),), 7))  # not divergence-free: the projection has work to do
    with _lib.options(**pre):
        ps = mkps()
        with _lib.options(**post):
            u, p = raw.clone(), f32.scalarfield32(sp)
            f32.project32_(u, sp, ps, p)
            hp = sha(label, u.cpu().numpy(), p.cpu().numpy())
            q = f32.to_f32(sp, randn(sp.grid.N, 9))
            ps(q)
            hs = sha(label, q.cpu().numpy())
            hd = sha(label, np.float32(f32.max_abs_divergence32(raw, sp, ps)))
    print(f"{label:58s} project={hp} solve={hs} maxdiv={hd}", flush=True)
    del ps


def run_f32_ext(label, geom, method, opts, temp=False, smag=False, with_force=False, wrap=None, nsteps=3, chained=False):
    f32 = ins.f32
    sp, mkps, u, t, dt = setup32(geom, with_force, temp, smag, wrap)
    with _lib.options(**opts):
        ps = mkps()
        cache = f32.ERKCache32(getattr(ins.RKMethods, method)(), sp, ps)
        kw = dict(temp=t, θ=0.17 if smag else None)
        if chained:
            f32.timesteps32_(cache, u, dt, nsteps, **kw)
        else:
            for _ in range(nsteps):
                f32.timestep32_(cache, u, dt, **kw)
        print(f"{label:58s} {sha(label, u.cpu().numpy(), *([t.cpu().numpy()] if temp else []))}", flush=True)
    del cache, ps


def run_ad32(label, geom, temp):
    """∂L/∂u0 (and ∂L/∂temp0) of L = Σu² (+ Σtemp²) after 3 RK44 steps of ad32.timesteps: the recomputation runs the shared Float32 combine"""
    sp, mkps, u, t, dt = setup32(geom, temp=temp)
    ps = mkps()
    m = ins.RKMethods.RK44()
    u.requires_grad_(True)
    if temp:
        t.requires_grad_(True)
    st = ins.ad32.timesteps(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u, temp=t), dt, 3)
    ((st.u * st.u).sum() + ((st.temp * st.temp).sum() if temp else 0.0)).backward()
    print(f"{label:58s} {sha(label, u.grad.cpu().numpy(), *([t.grad.cpu().numpy()] if temp else []))}", flush=True)
    del st, ps


def cases_f32():
    """the Float32 solver routes, the extended loop, the adjoint's recomputation and the wrapped solver on periodic boxes (csrc/ins_f32.hip)"""
    boxes = (("hipfft", "per32x32"), ("hipfft", "per66x12x10"), ("hipfft", "per24x18"), ("fp64spectra", "per128x16x16"), ("fp64spectra", "per32x16x16"),
             ("float2", "per128x16x256"), ("float2", "per256x16x192"), ("wrapped", "walls24"))
    for route, geom in boxes:
        yield f"f32 solver {route} {geom}", run_f32_solver, dict(geom=geom, pre={}, post={})
    for name, pre, post in (("fp64spectra=1", dict(INS_F32_FP64_SPECTRA=1), {}), ("hipfftproject=1", dict(INS_F32_HIPFFT_PROJECT=1), {}),
                            ("splitgradient=1", {}, dict(INS_F32_SPLIT_GRADIENT=1))):
        yield f"f32 solver per128x16x256 {name}", run_f32_solver, dict(geom="per128x16x256", pre=pre, post=post)
    terms = (("temp", dict(temp=True)), ("smag", dict(smag=True)), ("force", dict(with_force=True)), ("all", dict(temp=True, smag=True, with_force=True)))
    for geom in ("per32x16x16", "per72x10x8", "walls24"):
        for method in ("RK44", "Wray3"):
            for what, kw in terms:
                yield f"f32 ext {what} {geom} {method}", run_f32_ext, dict(geom=geom, method=method, opts={}, **kw)
            yield f"f32 ext all {geom} {method} tempsplit", run_f32_ext, dict(geom=geom, method=method, opts=dict(INS_DISABLE_TEMP32_STAGE=1), temp=True,
                                                                              smag=True, with_force=True)
    for geom in ("per32x16x16", "walls24"):
        for temp in (False, True):
            yield f"f32 ad32.timesteps gradient {geom}{' temp' if temp else ''}", run_ad32, dict(geom=geom, temp=temp)
    for geom in ("per32x16x16", "per32x32"):  # ADVICE.md, first finding: pinned as it is, not as it should be
        yield f"f32 wrap32(spectral) {geom} RK44 (ADVICE.md defect: no ghost fills)", run_f32_ext, dict(geom=geom, method="RK44", opts={},
                                                                                                      wrap=ins.psolver_spectral)


def cases():
    per3 = [f"per{n}" for n in ("32x32x32", "66x10x4", "128x16x12", "128x16x16")]
    for with_force in (False, True):
        ff = "+force" if with_force else ""
        for geom in per3:  # fp64 3-D periodic: 62-wide, 64-wide (one / two wavefronts per row); on the last the stage kernel writes the right-hand side
            for method in ("RK44", "Wray3", "SSP33", "FE11"):
                for mode, base in (("single", {}), ("chain3", {}), ("graph4", dict(INS_STEP_GRAPH=1))):
                    for vn, vo in VARIANTS:
                        yield f"f64 {geom}{ff} {method} {mode} {vn}", run_f64, dict(geom=geom, method=method, mode=mode, opts={**base, **vo}, with_force=with_force)
        for method in ("RK44", "SSP33"):  # fp64 2-D periodic
            for mode in ("single", "chain3"):
                for vn, vo in VARIANTS:
                    yield f"f64 per64x32{ff} {method} {mode} {vn}", run_f64, dict(geom="per64x32", method=method, mode=mode, opts=vo, with_force=with_force)
        for geom in ("cavity64", "cavity72", "channel64", "channel72", "dirichlet2d12"):  # tiled (62- / 64-wide masked kernels) and generic kernel
            for vn, vo in VARIANTS:
                yield f"f64 {geom}{ff} RK44 single {vn}", run_f64, dict(geom=geom, method="RK44", mode="single", opts=vo, with_force=with_force)
        yield f"f64 lidbc12{ff} RK44 single (time-dependent walls)", run_f64, dict(geom="lidbc12", method="RK44", mode="single", opts={}, with_force=with_force)
        yield f"f64 cavity64{ff} RK44 single nofuse (reference order)", run_f64, dict(geom="cavity64", method="RK44", mode="single",
                                                                                     opts=dict(INS_DISABLE_FUSED_RK=1), with_force=with_force)
    # the extended loop: fused periodic (default / split temperature stage), tiled on a wall-bounded box, the any-grid loop on a 2-D box
    for what, kw in (("smag", dict(smag=True)), ("temp", dict(temp=True)), ("both", dict(smag=True, temp=True))):
        for with_force in (False, True):
            ff = "+force" if with_force else ""
            for method in ("RK44", "Wray3"):
                for vn, vo in VARIANTS + (("split", dict(INS_EXT_TEMP_SPLIT=1)), ("refseq", dict(INS_DISABLE_EXT_FUSED=1))):
                    yield f"ext {what}{ff} per72x10x8 {method} {vn}", run_f64, dict(geom="per72x10x8", method=method, mode="single", opts=vo, with_force=with_force, **kw)
            yield f"ext {what}{ff} per64x32 RK44 (any-grid loop)", run_f64, dict(geom="per64x32", method="RK44", mode="single", opts={}, with_force=with_force, **kw)
        if what == "smag":  # the temperature equation of this tool has periodic boundary data
            for with_force in (False, True):
                yield f"ext smag{'+force' if with_force else ''} walls24 RK44 (tiled)", run_f64, dict(geom="walls24", method="RK44", mode="single", opts={},
                                                                                                   with_force=with_force, smag=True)
    # the host stage loops: a user closure (only the host can call it), and the low-storage scheme natively and behind INS_HOST_STAGE_LOOP=1
    for geom in ("per32x32x32", "per64x32", "walls24"):
        yield f"host user-closure {geom} RK44 single", run_f64, dict(geom=geom, method="RK44", mode="single", opts={}, user=True)
        for mode in ("single", "chain3"):
            yield f"lmwray3 {geom} {mode} native", run_f64, dict(geom=geom, method="LMWray3", mode=mode, opts={})
            yield f"lmwray3 {geom} {mode} INS_HOST_STAGE_LOOP=1", run_f64, dict(geom=geom, method="LMWray3", mode=mode, opts={}, host_loop=True)
    wx, wbc, _ = geometry("walls24")
    for vn, vo in VARIANTS:
        yield f"f32 per128x16x256 RK44 single {vn}", run_f32, dict(x=exact((128, 16, 256)), bc=None, method="RK44", nsteps=3, chained=False, opts=vo)
        yield f"f32 per128x16x256 RK44 chain3 {vn}", run_f32, dict(x=exact((128, 16, 256)), bc=None, method="RK44", nsteps=3, chained=True, opts=vo)
        yield f"f32 per128x16x16 Wray3 chain3 {vn}", run_f32, dict(x=exact((128, 16, 16)), bc=None, method="Wray3", nsteps=3, chained=True, opts=vo)
    yield "f32 per32x16x16 RK44 single (narrow: plain kernels)", run_f32, dict(x=exact((32, 16, 16)), bc=None, method="RK44", nsteps=3, chained=False, opts={})
    yield "f32 walls24 RK44 single (wrapped fp64 solver)", run_f32, dict(x=wx, bc=wbc, method="RK44", nsteps=3, chained=False, opts={})
    yield from cases_f32()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="regex on the case label")
    a = ap.parse_args()
    _lib.load().ins_dbg_ext_fused_steps.restype = C.c_longlong
    S = Setups()
    n = 0
    for label, fn, kw in cases():
        if a.only and not re.search(a.only, label):
            continue
        try:
            fn(*((S, label) if fn is run_f64 else (label,)), **kw)
        except (_lib.INSHipError, ValueError, NotImplementedError) as e:  # a refusal of the library is an outcome like a hash
            print(f"{label:58s} refused: {type(e).__name__}: {e}", flush=True)
        n += 1
    print(f"# {n} cases, library {_lib.LIB_PATH if os.environ.get('INS_HIP_LIB') else 'of the tree'}")
    if NONFINITE:
        print(f"# {len(NONFINITE)} cases left non-finite fields: {NONFINITE}")
    return 1 if NONFINITE else 0


if __name__ == "__main__":
    sys.exit(main())
