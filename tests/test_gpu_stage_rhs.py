"""The stage kernel writes the Poisson right-hand side Ω·div(u*) itself (csrc/ins_flux64.hip, RHS) and the solver's x pass reads that one
array (XSRC_PI) instead of the three components of u* (XSRC_DIV).  INS_DISABLE_STAGE_RHS=1 restores the old route; every test asserts
through ins_dbg_stage_rhs_used / ins_dbg_stage_rhs that the new one really ran, so a silent fallback cannot pass.

Boxes: the smallest that select each code path of the route.
  128x16x16  two wavefronts per row; one z-chunk per tile column, so the plane below the chunk is the periodic wrap; 128 columns is also the one
             width whose non-correcting first stage runs on this kernel (wider even rows take the two-columns-per-lane kernel there)
  256x16x32  four wavefronts per row (the benchmark's tile shape; with INS_FLUX64_NW=8 also its eight-wavefront workgroup: two wavefront rows),
             several y tiles, eight z-chunks
  192x32x16  radix-3 x length: three wavefronts per row
  128x32x96  3·2^m z length, chunk borders inside the box, three different side lengths (an axis mix-up shows)
Spacings 2^-6, 2^-5, 2^-7: exactly uniform (the constant-record kernels) and different per direction, so the three 1/Δ differ.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-10  # multi-step RK against the oracle, relative L2: the bound of the stage-loop parity tests (tests/test_gpu_parity.py)

BOXES = [(128, 16, 16), (256, 16, 32), (192, 32, 16), (128, 32, 96)]
CASES = [(n, 0) for n in BOXES] + [((256, 16, 32), 8)]  # (box, INS_FLUX64_NW)
IDS = ["x".join(map(str, n)) + (f"-nw{nw}" if nw else "") for n, nw in CASES]
H = (2.0**-6, 2.0**-5, 2.0**-7)


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


@pytest.fixture()
def opts(ins):
    """set run-time options for one test; everything goes back to 0 afterwards"""
    from ins_amd import _lib

    touched = set()

    def set_(name, value):
        touched.add(name)
        _lib.set_option(name, value)

    yield set_
    for name in touched:
        _lib.set_option(name, 0)


def coords(n):
    return tuple(np.arange(ni + 1) * h for ni, h in zip(n, H))


def rell2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / max(np.sqrt(np.sum(b**2)), 1e-300))


def start_field(ins, sp, n, seed, psolver=None):
    """random_field plus a smooth Taylor-Green term, ghost volumes filled"""
    a = ins.to_numpy(ins.random_field(sp, kp=2, psolver=psolver, seed=seed))
    x, y, z = (2 * np.pi * (np.arange(ni + 2) - 1) / ni for ni in n)
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    a[..., 0] += 0.5 * np.sin(X) * np.cos(Y) * np.cos(Z)
    a[..., 1] -= 0.5 * np.cos(X) * np.sin(Y) * np.cos(2 * Z)
    a[..., 2] += 0.25 * np.cos(X) * np.cos(Y) * np.sin(Z)
    return ins.apply_bc_u_(ins.from_numpy(sp, a), 0.0, sp)


def rhs_launches(cache):
    from ins_amd import _lib

    k = C.c_int64(0)
    _lib.call("ins_dbg_stage_rhs_used", cache.handle, C.byref(k))
    return k.value


def step_pressure(ins, cache, sp):
    """the pressure the last step left in the integrator (padded scalar field), on the host"""
    import torch

    from ins_amd import _lib

    ptr = C.c_void_p()
    _lib.call("ins_rk_pressure", cache.handle, C.byref(ptr))
    torch.cuda.synchronize()
    out = np.empty(int(np.prod(sp.grid.N)), dtype=np.float64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
    return out.reshape(sp.grid.N, order="F")


@pytest.mark.parametrize("corr", [1, 0])
@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_right_hand_side_is_the_scaled_divergence_of_the_stored_stage_velocity(ins, opts, n, nw, corr):
    """One stage launch; the buffer against scalewithvolume(divergence(u*)) of the u* the same launch stored, at 1e-13·max|rhs| (not bitwise: two
    kernels, two contraction patterns).  Every epilogue term is present: ustart, the stencil input itself (self_in), one stage term.
    corr 1: the correcting kernel on every box.  corr 0: only 128-wide boxes launch this kernel for a non-correcting stage; elsewhere the
    route must say so (used == 0) and the old x pass stays."""
    import torch

    from ins_amd import _lib

    if nw:
        opts("INS_FLUX64_NW", nw)
    sp = ins.Setup(x=coords(n), Re=500.0)
    assert _lib.load().ins_grid_is_uniform_exact(sp.handle)
    psp = ins.psolver_spectral(sp)
    eng = C.c_int32(-1)
    _lib.call("ins_poisson_fft_engine", psp.handle, C.byref(eng))
    assert eng.value == 1  # own-FFT route
    m = ins.RKMethods.RK44()
    cache = ins.ode_method_cache(m, sp, psp)
    u_in = start_field(ins, sp, n, 11)
    ustart = start_field(ins, sp, n, 12)
    kterm = start_field(ins, sp, n, 13)
    g = torch.Generator(device="cpu").manual_seed(14)
    p = (0.05 * torch.randn(n[2], n[1], n[0], dtype=torch.float64, generator=g)).to(sp.device)  # unpadded, i fastest
    ustar = ins.vectorfield(sp)
    rhs = torch.zeros(n[2], n[1], n[0], dtype=torch.float64, device=sp.device)
    used = C.c_int32(-1)
    _lib.call("ins_dbg_stage_rhs", cache.handle, 1.0 / sp.Re, sp.ptr(u_in, True), C.c_void_p(p.data_ptr()) if corr else None, sp.ptr(ustart, True),
              sp.ptr(kterm, True), 0.37, 0.6, 0.01, sp.ptr(ustar, True), C.c_void_p(rhs.data_ptr()), C.byref(used), sp.stream)
    torch.cuda.synchronize()
    expect_used = 1 if (corr or n[0] == 128) else 0
    assert used.value == expect_used
    if not used.value:
        return
    ins.apply_bc_u_(ustar, 0.0, sp)
    want = ins.to_numpy(ins.scalewithvolume(ins.divergence(ustar, sp), sp))[1:-1, 1:-1, 1:-1]
    got = rhs.cpu().numpy().transpose(2, 1, 0)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"rhs {n} nw={nw} corr={corr}: max|rhs| = {scale:.3e}, max err = {err:.3e}")
    assert scale > 0 and err <= 1e-13 * scale


def run_steps(ins, sp, psp, m, u0, dt, chained):
    """one `timestep_`, or `timesteps_` with 3 chained steps; returns (u with ghosts, p, divergence, stage kernels that wrote the rhs)"""
    cache = ins.ode_method_cache(m, sp, psp)
    st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
    st = ins.timesteps_(m, st, dt, 3, cache=cache) if chained else ins.timestep_(m, st, dt, cache=cache)
    return ins.to_numpy(st.u), step_pressure(ins, cache, sp), ins.max_abs_divergence(st.u, sp), rhs_launches(cache)


@pytest.mark.parametrize("force", [False, True], ids=["noforce", "force"])
@pytest.mark.parametrize("method", ["RK44", "Wray3", "SSP33", "FE11"])
@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_whole_steps_equal_the_old_route(ins, opts, n, nw, method, force):
    """`timestep_` and 3 chained `timesteps_` with the route on against INS_DISABLE_STAGE_RHS=1: u with its ghost volumes and p at 1e-13 relative (the
    bound of test_chained_steps_equal_single_steps), and the divergence of the result no larger than twice the old route's."""
    if nw:
        opts("INS_FLUX64_NW", nw)
    kw = {}
    if force:
        kw["bodyforce"] = lambda a, x, y, z, t: (0.3 * np.sin(2 * np.pi * y / (n[1] * H[1])) + 0 * x + 0 * z) if a == 0 else 0 * (x + y + z)
    sp = ins.Setup(x=coords(n), Re=500.0, **kw)
    psp = ins.psolver_spectral(sp)
    m = getattr(ins.RKMethods, method)()
    u0 = start_field(ins, sp, n, 21, psolver=psp)
    ns = len(m.b)
    for chained in (False, True):
        u_new, p_new, div_new, k_new = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_RHS", 1)
        u_old, p_old, div_old, k_old = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_RHS", 0)
        assert k_old == 0
        # every correcting stage takes the route (stages >= 2, and the first stage of a chained step after the first: no chain with a force or one stage);
        # a non-correcting stage only on 128-wide boxes; never the last stage of a step that is not chained to its predecessor: it stores u* over its ustart
        nsteps = 3 if chained else 1
        want_k = 0
        for step in range(nsteps):
            raw_in = chained and ns > 1 and not force and step > 0
            for i in range(ns):
                corr = ns > 1 and (i > 0 or raw_in)
                in_place = ns > 1 and i == ns - 1 and not raw_in
                want_k += 1 if ((corr or n[0] == 128) and not in_place) else 0
        assert k_new == want_k, (k_new, want_k)
        eu, ep = rell2(u_new, u_old), rell2(p_new, p_old)
        print(f"step {n} nw={nw} {method} force={force} chained={chained}: rel u {eu:.2e}, rel p {ep:.2e}, div {div_new:.2e} (old {div_old:.2e})")
        assert eu < 1e-13 and ep < 1e-13
        assert div_new <= 2 * div_old


@pytest.mark.parametrize("n", BOXES[:2], ids=IDS[:2])
def test_rk44_matches_the_oracle(ins, oracle, n):
    o = oracle
    so = o.make_setup(coords(n), Re=500.0)
    sp = ins.Setup(x=coords(n), Re=500.0)
    pso, psp = o.psolver_spectral(so), ins.psolver_spectral(sp)
    u0 = o.random_field(so, kp=2, seed=5, psolver=pso)
    m = ins.RKMethods.RK44()
    cache = ins.ode_method_cache(m, sp, psp)
    st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.from_numpy(sp, u0), t=0.0)
    st = ins.timesteps_(m, st, 2e-3, 2, cache=cache)
    assert rhs_launches(cache) > 0
    want = o.solve_unsteady(so, (0.0, 4e-3), u0, method=o.RK44(), psolver=pso, dt=2e-3)["u"]
    assert rell2(ins.to_numpy(st.u), want) < STEP_TOL


def test_unchained_steps_on_a_box_of_many_workgroups(ins, opts):
    """Single `timestep_` calls store the last stage's u* over the caller's u, which is also that stage's ustart: a stage kernel that formed the right-hand
    side there would read neighbouring cells another workgroup may already have overwritten (it showed only on boxes of many workgroups, as a result
    that was no longer divergence-free).  That stage keeps the old route; four steps equal the old route and stay divergence-free."""
    n = (128, 64, 64)
    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    m = ins.RKMethods.RK44()
    u0 = start_field(ins, sp, n, 31, psolver=psp)
    res = {}
    for off in (0, 1):
        opts("INS_DISABLE_STAGE_RHS", off)
        cache = ins.ode_method_cache(m, sp, psp)
        st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
        for _ in range(4):
            st = ins.timestep_(m, st, 2e-3, cache=cache)
        res[off] = (ins.to_numpy(st.u), ins.max_abs_divergence(st.u, sp), rhs_launches(cache))
    assert res[0][2] == 4 * 3 and res[1][2] == 0  # stages 1-3 of every step (128 columns: the first stage too), not the fourth
    print(f"unchained 128x64x64: rel u {rell2(res[0][0], res[1][0]):.2e}, div {res[0][1]:.2e} (old {res[1][1]:.2e})")
    assert rell2(res[0][0], res[1][0]) < 1e-13
    assert res[0][1] <= 2 * res[1][1]
