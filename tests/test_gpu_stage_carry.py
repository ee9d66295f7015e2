"""RK44's second stage carries the part of the last stage's combination it has in registers forward (csrc/ins_rk_terms.h, RkCarryPlan; csrc/ins_flux64.hip,
CARRY): it also stores S = -1/3 ustart + 1/3 V_0 + 2/3 V_1, and the last stage starts from S instead of loading ustart, V_0 and V_1.
INS_DISABLE_STAGE_CARRY=1 restores the old combination; every test asserts through ins_dbg_stage_carry_used that the route really ran (one carrying launch per
RK44 step, none for a method without a plan), so a silent fallback cannot pass.  The sum is re-associated (S is rounded once when it is stored), so the two
routes agree at the 1e-16 level, not bit for bit: the bound is 1e-13 relative L2, that of test_chained_steps_equal_single_steps.

Boxes (those of tests/test_gpu_stage_rhs.py, and one the right-hand-side route does not take):
  128x16x16  two wavefronts per row; one z-chunk per tile column, so the plane below the chunk is the periodic wrap
  256x16x32  four wavefronts per row (the benchmark's tile shape; with INS_FLUX64_NW=8 also its eight-wavefront workgroup: two wavefront rows)
  192x32x16  three wavefronts per row
  96x16x16   a workgroup does not span a row (the second wavefront is half outside the box): the correcting kernel without the right-hand-side route
Spacings 2^-6, 2^-5, 2^-7: exactly uniform and different per direction.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP_TOL = 1e-10  # multi-step RK against the oracle, relative L2: the bound of the stage-loop parity tests (tests/test_gpu_parity.py)
ROUTE_TOL = 1e-13  # route on against route off, relative L2

BOXES = [(128, 16, 16), (256, 16, 32), (192, 32, 16), (96, 16, 16)]
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


def run_steps(ins, sp, psp, m, u0, dt, chained):
    """one `timestep_`, or `timesteps_` with 3 chained steps; returns (u with ghosts, p, divergence, carrying launches, stage kernels that wrote the rhs)"""
    cache = ins.ode_method_cache(m, sp, psp)
    st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
    st = ins.timesteps_(m, st, dt, 3, cache=cache) if chained else ins.timestep_(m, st, dt, cache=cache)
    return (ins.to_numpy(st.u), step_pressure(ins, cache, sp), ins.max_abs_divergence(st.u, sp), counter(cache, "ins_dbg_stage_carry_used"),
            counter(cache, "ins_dbg_stage_rhs_used"))


def on_against_off(ins, opts, sp, psp, m, u0, label, planned_per_step):
    for chained in (False, True):
        u_new, p_new, div_new, k_new, r_new = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_CARRY", 1)
        u_old, p_old, div_old, k_old, r_old = run_steps(ins, sp, psp, m, u0, 2e-3, chained)
        opts("INS_DISABLE_STAGE_CARRY", 0)
        eu, ep = rell2(u_new, u_old), rell2(p_new, p_old)
        print(f"{label} chained={chained}: carrying launches {k_new} (off: {k_old}), rel u {eu:.2e}, rel p {ep:.2e}, div {div_new:.2e} (old {div_old:.2e})")
        assert k_old == 0
        assert k_new == planned_per_step * (3 if chained else 1), k_new
        assert r_new == r_old  # which stages write the Poisson right-hand side does not depend on the plan
        assert eu < ROUTE_TOL and ep < ROUTE_TOL
        assert div_new <= 2 * div_old


@pytest.mark.parametrize("force", [False, True], ids=["noforce", "force"])
@pytest.mark.parametrize("method", ["RK44", "Wray3", "SSP33", "FE11"])
@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_whole_steps_equal_the_old_combination(ins, opts, n, nw, method, force):
    """`timestep_` and 3 chained `timesteps_` with the route on against INS_DISABLE_STAGE_CARRY=1: u with its ghost volumes and p at 1e-13 relative, the
    divergence of the result no larger than twice the old route's, and exactly the carrying launches the plan predicts."""
    if nw:
        opts("INS_FLUX64_NW", nw)
    kw = {}
    if force:
        kw["bodyforce"] = lambda a, x, y, z, t: (0.3 * np.sin(2 * np.pi * y / (n[1] * H[1])) + 0 * x + 0 * z) if a == 0 else 0 * (x + y + z)
    sp = ins.Setup(x=coords(n), Re=500.0, **kw)
    psp = ins.psolver_spectral(sp)
    m = getattr(ins.RKMethods, method)()
    u0 = start_field(ins, sp, n, 21, psolver=psp)
    on_against_off(ins, opts, sp, psp, m, u0, f"carry {n} nw={nw} {method} force={force}", 1 if method == "RK44" else 0)


@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_route_without_the_stage_right_hand_side(ins, opts, n, nw):
    """INS_DISABLE_STAGE_RHS=1: every box runs the correcting kernel's plain form, which carries as well."""
    if nw:
        opts("INS_FLUX64_NW", nw)
    opts("INS_DISABLE_STAGE_RHS", 1)
    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    u0 = start_field(ins, sp, n, 22, psolver=psp)
    on_against_off(ins, opts, sp, psp, ins.RKMethods.RK44(), u0, f"carry, no stage rhs {n} nw={nw}", 1)


@pytest.mark.parametrize("n,nw", CASES, ids=IDS)
def test_route_under_the_step_graph(ins, opts, n, nw):
    """INS_STEP_GRAPH=1, 6 chained steps: the replayed steps are those of the plain loop bit for bit (the buffers of the plan are fixed per integrator),
    and equal the old combination at 1e-13.  Replayed steps enqueue nothing, so the counter only has to show that the captured step carried."""
    import torch

    from ins_amd import _lib

    if nw:
        opts("INS_FLUX64_NW", nw)
    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    m = ins.RKMethods.RK44()
    u0 = start_field(ins, sp, n, 23, psolver=psp)
    fn = _lib.load().ins_dbg_rk_graph_replays
    fn.restype, fn.argtypes = C.c_longlong, [C.c_void_p]

    def run():
        cache = ins.ode_method_cache(m, sp, psp)
        st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
        st = ins.timesteps_(m, st, 2e-3, 6, cache=cache)
        torch.cuda.synchronize()
        return ins.to_numpy(st.u), ins.max_abs_divergence(st.u, sp), counter(cache, "ins_dbg_stage_carry_used"), int(fn(cache.handle))

    u_plain, _, k_plain, r_plain = run()
    opts("INS_STEP_GRAPH", 1)
    u_graph, div_graph, k_graph, r_graph = run()
    opts("INS_DISABLE_STAGE_CARRY", 1)
    u_old, div_old, k_old, r_old = run()
    print(f"carry under the graph {n} nw={nw}: launches {k_plain} plain, {k_graph} graph, replays {r_graph}, rel u {rell2(u_graph, u_old):.2e}")
    assert k_plain == 6 and r_plain == 0
    assert r_graph > 0 and r_old == r_graph and 1 <= k_graph <= 6 - r_graph + 1 and k_old == 0  # direct steps and the one captured
    assert np.array_equal(u_graph, u_plain)
    assert rell2(u_graph, u_old) < ROUTE_TOL
    assert div_graph <= 2 * div_old


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
    assert counter(cache, "ins_dbg_stage_carry_used") > 0
    want = o.solve_unsteady(so, (0.0, 4e-3), u0, method=o.RK44(), psolver=pso, dt=2e-3)["u"]
    err = rell2(ins.to_numpy(st.u), want)
    print(f"carry against the oracle {n}: rel L2 {err:.2e}")
    assert err < STEP_TOL


def test_unchained_steps_on_a_box_of_many_workgroups(ins, opts):
    """Four single `timestep_` calls on a box of many workgroups: S is stored while other workgroups still read the halo rows and planes of the stage's inputs,
    and the stage between stores over a dead stage velocity.  A buffer mix-up shows here as a result that is no longer divergence-free or leaves the old one."""
    n = (128, 64, 64)
    sp = ins.Setup(x=coords(n), Re=500.0)
    psp = ins.psolver_spectral(sp)
    m = ins.RKMethods.RK44()
    u0 = start_field(ins, sp, n, 31, psolver=psp)
    res = {}
    for off in (0, 1):
        opts("INS_DISABLE_STAGE_CARRY", off)
        cache = ins.ode_method_cache(m, sp, psp)
        st = ins.create_stepper(m, setup=sp, psolver=psp, u=ins.copyfield(u0), t=0.0)
        for _ in range(4):
            st = ins.timestep_(m, st, 2e-3, cache=cache)
        res[off] = (ins.to_numpy(st.u), ins.max_abs_divergence(st.u, sp), counter(cache, "ins_dbg_stage_carry_used"))
    assert res[0][2] == 4 and res[1][2] == 0
    print(f"carry, unchained 128x64x64: rel u {rell2(res[0][0], res[1][0]):.2e}, div {res[0][1]:.2e} (old {res[1][1]:.2e})")
    assert rell2(res[0][0], res[1][0]) < ROUTE_TOL
    assert res[0][1] <= 2 * res[1][1]
