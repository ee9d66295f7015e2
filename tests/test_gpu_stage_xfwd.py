"""The correcting stage kernel of 256-wide boxes stores the half-complex x-spectrum of the Poisson right-hand side (csrc/ins_flux64.hip, XF) and the
solve starts at its y pass; INS_DISABLE_STAGE_XFWD=1 restores the real-space array and the x-forward pass.  Every test asserts through
ins_dbg_stage_xfwd_used / ins_dbg_stage_xfwd that the route really ran, so a silent fallback cannot pass.

Boxes (spacings 2^-6, 2^-5, 2^-7 as in tests/test_gpu_stage_rhs.py):
  256x16x32  four wavefronts per row; INS_FLUX64_NW default (4: one wavefront row per workgroup) and 8 (two); several y tiles; eight z-chunks of four planes, so
             every chunk drains its two lagging planes and one chunk starts at the periodic wrap
  256x16x16  chunks of four planes on the shortest z side the own-FFT solver takes: the drain is a third of every chunk's iterations.  (The issue named
             256x8x4 for this; the own-FFT passes start at 16 points per side, so that box solves on rocFFT and neither right-hand-side route exists on it.)
  128x16x16, 192x32x16  two and three wavefronts per row: the route refuses them (used == 0) and the steps are those of the old route, bit for bit.
A wavefront row outside the box (the early-return path's barrier count) needs n1 % 4 == 2 at INS_FLUX64_NW=8; every side the own-FFT solver takes (powers of
two from 16, 3 * 2^m, 5 * 2^m from 96 / 160) is a multiple of 4, so no such box exists.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-10  # multi-step RK against the oracle, relative L2 (tests/test_gpu_parity.py)

BOX = (256, 16, 32)
CASES = [(BOX, 0), (BOX, 8), ((256, 16, 16), 0)]  # (box, INS_FLUX64_NW)
IDS = ["x".join(map(str, n)) + (f"-nw{nw}" if nw else "") for n, nw in CASES]
REFUSED = [(128, 16, 16), (192, 32, 16)]
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


def counter(cache, name):
    from ins_amd import _lib

    k = C.c_int64(0)
    _lib.call(name, cache.handle, C.byref(k))
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


def one_launch(ins, n, entry, out):
    """one correcting stage launch with every epilogue term (ustart, the stencil input itself, one stage term); returns `used`"""
    import torch

    from ins_amd import _lib

    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    eng = C.c_int32(-1)
    _lib.call("ins_poisson_fft_engine", psp.handle, C.byref(eng))
    assert eng.value == 1  # own-FFT route
    cache = ins.ode_method_cache(ins.RKMethods.RK44(), sp, psp)
    u_in = start_field(ins, sp, n, 11)
    ustart = start_field(ins, sp, n, 12)
    kterm = start_field(ins, sp, n, 13)
    g = torch.Generator(device="cpu").manual_seed(14)
    p = (0.05 * torch.randn(n[2], n[1], n[0], dtype=torch.float64, generator=g)).to(sp.device)  # unpadded, i fastest
    ustar = ins.vectorfield(sp)
    used = C.c_int32(-1)
    _lib.call(entry, cache.handle, 1.0 / sp.Re, sp.ptr(u_in, True), C.c_void_p(p.data_ptr()), sp.ptr(ustart, True), sp.ptr(kterm, True), 0.37, 0.6, 0.01,
              sp.ptr(ustar, True), C.c_void_p(out.data_ptr()), C.byref(used), sp.stream)
    torch.cuda.synchronize()
    return used.value


@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_stored_spectrum_is_the_x_transform_of_the_right_hand_side(ins, opts, n, nw):
    """One stage launch on each route, same inputs: the spectrum rows against numpy.fft.rfft along x of the right-hand side ins_dbg_stage_rhs returns, at
    1e-13 · max|spectrum| · log2(256).  Columns 129 .. 135 of a row are padding and are not compared."""
    import torch

    if nw:
        opts("INS_FLUX64_NW", nw)
    dev = ins.Setup(x=coords(n), Re=500.0).device
    kxs = (n[0] // 2 + 1 + 7) & ~7
    rhs = torch.zeros(n[2], n[1], n[0], dtype=torch.float64, device=dev)
    spec = torch.zeros(n[2], n[1], kxs, 2, dtype=torch.float64, device=dev)
    assert one_launch(ins, n, "ins_dbg_stage_rhs", rhs) == 1
    assert one_launch(ins, n, "ins_dbg_stage_xfwd", spec) == 1
    want = np.fft.rfft(rhs.cpu().numpy(), axis=2)
    got = torch.view_as_complex(spec).cpu().numpy()[:, :, : n[0] // 2 + 1]
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print(f"spectrum {n} nw={nw}: max|spectrum| = {scale:.3e}, max err = {err:.3e}, bound {1e-13 * scale * 8:.3e}")
    assert scale > 0 and err <= 1e-13 * scale * np.log2(256)


@pytest.mark.parametrize("n", REFUSED, ids=["x".join(map(str, n)) for n in REFUSED])
def test_other_row_widths_keep_the_array(ins, n):
    import torch

    dev = ins.Setup(x=coords(n), Re=500.0).device
    kxs = (n[0] // 2 + 1 + 7) & ~7
    spec = torch.zeros(n[2], n[1], kxs, 2, dtype=torch.float64, device=dev)
    assert one_launch(ins, n, "ins_dbg_stage_xfwd", spec) == 0
    assert float(spec.abs().max()) == 0.0


def run_steps(ins, sp, psp, m, u0, dt, chained):
    """one `timestep_`, or `timesteps_` with 3 chained steps; returns (u with ghosts, p, divergence, launches that formed the rhs, launches that stored the spectrum)"""
    cache = ins.ode_method_cache(m, sp, psp)
    st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
    st = ins.timesteps_(m, st, dt, 3, cache=cache) if chained else ins.timestep_(m, st, dt, cache=cache)
    return (ins.to_numpy(st.u), step_pressure(ins, cache, sp), ins.max_abs_divergence(st.u, sp), counter(cache, "ins_dbg_stage_rhs_used"),
            counter(cache, "ins_dbg_stage_xfwd_used"))


@pytest.mark.parametrize("force", [False, True], ids=["noforce", "force"])
@pytest.mark.parametrize("method", ["RK44", "Wray3", "SSP33", "FE11"])
@pytest.mark.parametrize("n,nw", CASES + [(n, 0) for n in REFUSED], ids=IDS + ["x".join(map(str, n)) for n in REFUSED])
def test_whole_steps_equal_the_array_route(ins, opts, n, nw, method, force):
    """`timestep_` and 3 chained `timesteps_` with the route on against INS_DISABLE_STAGE_XFWD=1: u with its ghost volumes and p at 1e-13 relative, the divergence
    of the result no larger than twice the other route's.  Boxes the route refuses: no launch of it, identical results."""
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
        u_new, p_new, div_new, r_new, k_new = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_XFWD", 1)
        u_old, p_old, div_old, r_old, k_old = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_XFWD", 0)
        assert k_old == 0
        # every correcting stage takes the route (stages >= 2, and the first stage of a chained step after the first: no chain with a force or one stage), never the
        # last stage of a step that is not chained to its predecessor: it stores u* over its ustart
        nsteps = 3 if chained else 1
        want_k = 0
        for step in range(nsteps):
            raw_in = chained and ns > 1 and not force and step > 0
            for i in range(ns):
                corr = ns > 1 and (i > 0 or raw_in)
                in_place = ns > 1 and i == ns - 1 and not raw_in
                want_k += 1 if (corr and not in_place and n[0] == 256) else 0
        assert k_new == want_k, (k_new, want_k)
        assert r_new == r_old  # the launches that formed the right-hand side, in either form
        eu, ep = rell2(u_new, u_old), rell2(p_new, p_old)
        print(f"step {n} nw={nw} {method} force={force} chained={chained}: rel u {eu:.2e}, rel p {ep:.2e}, div {div_new:.2e} (other {div_old:.2e}), launches {k_new}")
        if n[0] != 256:
            assert np.array_equal(u_new, u_old) and np.array_equal(p_new, p_old)
        assert eu < 1e-13 and ep < 1e-13
        assert div_new <= 2 * div_old


def test_rk44_matches_the_oracle(ins, oracle):
    n = BOX
    o = oracle
    so = o.make_setup(coords(n), Re=500.0)
    sp = ins.Setup(x=coords(n), Re=500.0)
    pso, psp = o.psolver_spectral(so), ins.psolver_spectral(sp)
    u0 = o.random_field(so, kp=2, seed=5, psolver=pso)
    m = ins.RKMethods.RK44()
    cache = ins.ode_method_cache(m, sp, psp)
    st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.from_numpy(sp, u0), t=0.0)
    st = ins.timesteps_(m, st, 2e-3, 2, cache=cache)
    assert counter(cache, "ins_dbg_stage_xfwd_used") > 0
    want = o.solve_unsteady(so, (0.0, 4e-3), u0, method=o.RK44(), psolver=pso, dt=2e-3)["u"]
    err = rell2(ins.to_numpy(st.u), want)
    print(f"oracle {n}: rel L2 {err:.2e}")
    assert err < STEP_TOL


def test_unchained_steps(ins, opts):
    """Four single `timestep_` calls: the last stage stores u* over the caller's u, which is also its ustart, and keeps the x pass; so does the first stage, which does
    not correct (it keeps the x pass that forms the divergence, as on the array route at this width).  Stages 2 and 3 store the spectrum: 4 x 2 launches.  (The issue
    wrote 4 x 3, the count of tests/test_gpu_stage_rhs.py's 128-wide box, whose first stage runs on this kernel too.)  Equal to the array route, divergence-free."""
    n = BOX
    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    m = ins.RKMethods.RK44()
    u0 = start_field(ins, sp, n, 31, psolver=psp)
    res = {}
    for off in (0, 1):
        opts("INS_DISABLE_STAGE_XFWD", off)
        cache = ins.ode_method_cache(m, sp, psp)
        st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
        for _ in range(4):
            st = ins.timestep_(m, st, 2e-3, cache=cache)
        res[off] = (ins.to_numpy(st.u), ins.max_abs_divergence(st.u, sp), counter(cache, "ins_dbg_stage_xfwd_used"))
    assert res[0][2] == 4 * 2 and res[1][2] == 0
    print(f"unchained {n}: rel u {rell2(res[0][0], res[1][0]):.2e}, div {res[0][1]:.2e} (other {res[1][1]:.2e})")
    assert rell2(res[0][0], res[1][0]) < 1e-13
    assert res[0][1] <= 2 * res[1][1]
    assert res[0][1] < 1e-10
