"""GPU: `ad.timesteps` (autodiff.py) and the native step pullback ins_rk_step_pullback_f64 (csrc/ins_rk_adjoint.hip).

  1. forward: bitwise the native multi-step loop with the same chunking; the input is untouched;
  2. gradient against `nsteps` calls of `ad.timestep` (the unrolled autograd path), ||g - g_ref|| <= TOL ||g_ref||;
  3. 32 rows of the dense transpose of one RK44 step against central differences of the native step;
  4. Taylor test through 20 RK44 steps: the central remainder falls by 8 per halving;
  5. peak memory grows by the extra checkpoints only;
  6. refusals;  7. nothing is saved without grad;  8. fused and two-launch reverse stages agree.
"""
import numpy as np
import pytest

from tests.test_gpu_adjoint import GEOMS, TOL, _u0, dot, mirror, nrm, rand, relmax, solvers
from tests.test_gpu_stage_rhs import coords, rhs_launches, start_field

pytestmark = pytest.mark.gpu

DT = 1e-3


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


METHODS = {
    "RK44": lambda ins: ins.RKMethods.RK44(),
    "RK33C2": lambda ins: ins.RKMethods.RK33C2(),   # three stages
    "LMWray3": lambda ins: ins.LMWray3(),
    "DOPRI6": lambda ins: ins.RKMethods.DOPRI6(),   # six stages: more terms in a reverse stage than the fused form takes
}

_cache = {}


def problem(ins, oracle, name):
    """(setup, solvers, u0, w) of a geometry, built once per module"""
    if name not in _cache:
        if name == "stage_rhs":  # the narrowest box whose chained forward runs the stage kernels that write the Poisson right-hand side
            n = (128, 16, 16)
            sp = ins.Setup(x=coords(n), Re=1000.0)
            pss = [ins.psolver_spectral(sp)]
            u0 = start_field(ins, sp, n, 5, psolver=pss[0])
        else:
            sp = mirror(ins, GEOMS[name](oracle), oracle)
            pss = solvers(ins, sp, name)
            u0 = _u0(ins, sp, pss[0], 80)
        _cache[name] = (sp, pss, u0, rand(ins, sp, True, 81))
    return _cache[name]


def loss(u, w):
    return 0.5 * (w * u * u).sum()


def grad_rollout(ins, method, sp, ps, u0, w, nsteps, every):
    import torch

    uu = u0.clone().requires_grad_(True)
    out = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, nsteps, checkpoint_every=every).u
    (g,) = torch.autograd.grad(loss(out, w), uu)
    return g


def grad_unrolled(ins, method, sp, ps, u0, w, nsteps, key=None):
    """the reference: nsteps calls of ad.timestep through torch autograd, computed once per key"""
    import torch

    if key is not None and key in _cache:
        return _cache[key]
    uu = u0.clone().requires_grad_(True)
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu)
    for _ in range(nsteps):
        st = ins.ad.timestep(method, st, DT)
    (g,) = torch.autograd.grad(loss(st.u, w), uu)
    if key is not None:
        _cache[key] = g
    return g


def rel(g, ref):
    return nrm(g - ref) / nrm(ref)


# ------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name,mname", [("periodic32_3d", "RK44"), ("mixed", "RK44"), ("box_pressure", "LMWray3"), ("periodic32_2d", "DOPRI6")])
def test_forward_is_the_native_loop(ins, oracle, name, mname):
    import torch

    sp, pss, u0, _ = problem(ins, oracle, name)
    ps, method = pss[0], METHODS[mname](ins)
    before = u0.clone()
    uu = u0.clone().requires_grad_(True)
    got = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, 5, checkpoint_every=2)
    assert got.u.grad_fn is not None and got.n == 5 and abs(got.t - 5 * DT) < 1e-15
    assert torch.equal(uu.detach(), before), "the input was changed"
    cache = ins.ode_method_cache(method, sp, ps)
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u0.clone())
    for n in (2, 2, 1):
        st = ins.timesteps_(method, st, DT, n, cache=cache)
    assert torch.equal(got.u.detach(), st.u), "not bitwise the native loop with the same chunking"
    one = ins.timesteps_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0.clone()), DT, 5, cache=cache).u
    assert float((got.u.detach() - one).abs().max()) <= 1e-13 * float(one.abs().max())
    # 7. nothing saved without grad: no graph, the same numbers
    with torch.no_grad():
        a = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, 5, checkpoint_every=2).u
    b = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), DT, 5, checkpoint_every=2).u
    assert a.grad_fn is None and b.grad_fn is None and not a.requires_grad and not b.requires_grad
    for x in (a, b):  # one native call instead of chunks: the chained loop differs from it by rounding at most
        assert float((x - got.u.detach()).abs().max()) <= 1e-13 * float(one.abs().max())
    assert torch.equal(a, one) and torch.equal(b, one)


# ------------------------------------------------------------------------------------ 2. gradient against the unrolled path
GEOM_CASES = ["box_periodic", "box_dirichlet", "box_symmetric", "box_pressure", "mixed", "periodic32_2d", "periodic32_3d", "stage_rhs"]
STEP_CASES = [(1, 1), (1, 2), (1, 5), (5, 1), (5, 2), (5, 5), (3, None)]


def check_gradient(ins, oracle, name, mname, nsteps, every, all_solvers=False):
    sp, pss, u0, w = problem(ins, oracle, name)
    method = METHODS[mname](ins)
    for q, ps in enumerate(pss if all_solvers else pss[:1]):
        ref = grad_unrolled(ins, method, sp, ps, u0, w, nsteps, key=(name, mname, nsteps, q))
        g = grad_rollout(ins, method, sp, ps, u0, w, nsteps, every)
        r = rel(g, ref)
        print(f"ad.timesteps vs unrolled: {name} {mname} nsteps={nsteps} every={every} solver={q}: rel = {r:.3e}")
        assert r <= TOL, (name, mname, nsteps, every, q, r)


@pytest.mark.parametrize("name", GEOM_CASES)
def test_gradient_matches_unrolled_geometries(ins, oracle, name):
    """RK44, five steps in chunks of two (a ragged last chunk), every solver the geometry has."""
    if name == "stage_rhs":
        sp, pss, u0, _ = problem(ins, oracle, name)
        method = METHODS["RK44"](ins)
        adj = ins.ad._step_adjoint(method, sp, pss[0])
        k0 = rhs_launches(adj.cache)
        uu = u0.clone().requires_grad_(True)
        ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=pss[0], u=uu), DT, 5, checkpoint_every=2)
        assert rhs_launches(adj.cache) > k0, "the chained forward did not take the stage kernels that write the Poisson right-hand side"
    check_gradient(ins, oracle, name, "RK44", 5, 2, all_solvers=True)


@pytest.mark.parametrize("mname", ["RK33C2", "LMWray3", "DOPRI6"])
@pytest.mark.parametrize("name", ["box_dirichlet", "periodic32_2d", "mixed"])
def test_gradient_matches_unrolled_methods(ins, oracle, name, mname):
    check_gradient(ins, oracle, name, mname, 5, 2)


@pytest.mark.parametrize("nsteps,every", STEP_CASES)
@pytest.mark.parametrize("name", ["box_pressure", "periodic32_3d"])
def test_gradient_matches_unrolled_chunkings(ins, oracle, name, nsteps, every):
    check_gradient(ins, oracle, name, "RK44", nsteps, every)


def test_gradient_with_steady_body_force(ins, oracle):
    so = GEOMS["box_dirichlet"](oracle)
    bcs = tuple((ins.DirichletBC(), ins.DirichletBC()) for _ in range(2))
    sp = ins.Setup(x=tuple(so.grid.x[a][1:-1] for a in range(2)), boundary_conditions=bcs, Re=so.Re,
                   bodyforce=lambda a, x, y, t: (3.0 * np.sin(2 * np.pi * y) + 0 * x) if a == 0 else (2.0 * np.cos(2 * np.pi * x) + 0 * y), issteadybodyforce=True)
    ps = ins.psolver_direct(sp)
    method = ins.RKMethods.RK44()
    u0, w = _u0(ins, sp, ps, 82), rand(ins, sp, True, 83)
    ref = grad_unrolled(ins, method, sp, ps, u0, w, 5)
    g = grad_rollout(ins, method, sp, ps, u0, w, 5, 2)
    # the force is in the forward and in the recomputation: without it the states differ at O(DT |f|) and so does the gradient
    sp0 = mirror(ins, so, oracle)
    g0 = grad_rollout(ins, method, sp0, ins.psolver_direct(sp0), u0, w, 5, 2)
    print(f"steady body force: rel = {rel(g, ref):.3e}; without the force {rel(g0, ref):.3e}")
    assert rel(g, ref) <= TOL and rel(g0, ref) > 1e3 * TOL


# ------------------------------------------------------------------------------------ 3. dense transpose of one step
@pytest.mark.parametrize("name", ["box_dirichlet", "box_pressure"])
def test_step_pullback_rows_match_central_differences(ins, oracle, name):
    """Rows of the step's Jacobian on the smallest box, by unit cotangents through ins_rk_step_pullback_f64, against central differences of the native step.

    tests/test_gpu_adjoint.py item 3 probes with unit vectors because its operators are linear or quadratic, for which a central difference is exact.
    One RK44 step is a polynomial of degree 16 in u, so the probe is chosen where both error terms of a central difference stay a decade under TOL:
    truncation h² |∂³u_out| / 6 with |∂³u_out| ~ Δt² / Δx² = 5e-9 at Δt = 1e-5, Δx = 1/7, and rounding eps |u| / (2h) with |u| ~ 3.  h = 2^-7 gives
    5e-14 and 4e-14.  At that Δt the momentum terms enter the Jacobian at Δt / Δx ~ 1e-4, eight digits above TOL; the ghost fills and the projection at 1."""
    import torch

    from ins_amd import _lib

    sp, pss, u0, _ = problem(ins, oracle, name)
    ps, method = pss[0], ins.RKMethods.RK44()
    dt, h = 1e-5, 2.0**-7
    adj = ins.ad._step_adjoint(method, sp, ps)
    cache = ins.ode_method_cache(method, sp, ps)
    N, D = tuple(sp.grid.N), sp.grid.dimension
    shape = N + (D,)
    n = int(np.prod(shape))

    def step(a):
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=ins.from_numpy(sp, a))
        return ins.to_numpy(ins.timestep_(method, st, dt, cache=cache).u).reshape(-1, order="F")

    base = ins.to_numpy(u0)
    J = np.empty((n, n))
    e = np.zeros(n)
    for m in range(n):
        e[m] = h
        d = e.reshape(shape, order="F")
        J[:, m] = (step(base + d) - step(base - d)) / (2 * h)
        e[m] = 0.0
    # 32 outputs: the corner and edge ghosts, the volumes next to each boundary, and interior ones, of both components
    idx = [(0, 0), (0, 3), (3, 0), (N[0] - 1, N[1] - 1), (N[0] - 1, 4), (4, N[1] - 1), (1, 1), (1, 4), (4, 1), (N[0] - 2, N[1] - 2), (N[0] - 2, 3),
           (3, N[1] - 2), (2, 2), (4, 4), (5, 3), (3, 5)]
    rows = [np.ravel_multi_index(ij + (a,), shape, order="F") for a in range(D) for ij in idx]
    assert len(rows) == 32
    got = np.empty((len(rows), n))
    for r, k in enumerate(rows):
        cot = np.zeros(n)
        cot[k] = 1.0
        ubar = ins.from_numpy(sp, cot.reshape(shape, order="F"))
        adj.step_pullback_(ubar, u0, dt)
        got[r] = ins.to_numpy(ubar).reshape(-1, order="F")
    err = relmax(got, J[rows])
    print(f"step pullback rows vs central differences, {name}: relmax = {err:.3e}")
    assert np.max(np.abs(J[rows])) > 0.5 and err <= TOL, err
    # ubar aliasing ustart is refused
    u = u0.clone()
    rc = _lib.load().ins_rk_step_pullback_f64(adj._handle, 1.0 / sp.Re, sp.ptr(u, True), None, dt, sp.ptr(u, True), sp.stream)
    assert rc == -1 and b"alias" in _lib.load().ins_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ 4. Taylor test
def test_taylor_through_20_steps(ins, oracle):
    """|L(u + hv) - L(u - hv) - 2h <g, v>| is the cubic remainder: it falls by 8 per halving of h, over h = 1e-2 / 2^k, k = 0..3 (the range of the
    Taylor tests of tests/test_gpu_adjoint.py, whose one-sided remainder falls by 4 +- 0.5)."""
    import torch

    sp, pss, u0, w = problem(ins, oracle, "periodic32_2d")
    ps, method = pss[0], ins.RKMethods.RK44()
    v = _u0(ins, sp, ps, 84)
    v = v * (nrm(u0) / nrm(v))
    uu = u0.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(loss(ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, 20).u, w), uu)
    dJ = dot(g, v)

    def L(e):
        with torch.no_grad():
            return float(loss(ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0 + e * v), DT, 20).u, w))

    hs = [1e-2 / 2**k for k in range(4)]
    r = [abs(L(h) - L(-h) - 2 * h * dJ) for h in hs]
    ratios = [r[k] / r[k + 1] for k in range(3)]
    print(f"Taylor remainders {r}, ratios {ratios}")
    assert all(abs(x - 8.0) <= 1.0 for x in ratios), (r, ratios)


# ------------------------------------------------------------------------------------ 5. memory
def test_peak_memory_grows_by_the_checkpoints_only(ins, oracle):
    import torch

    sp, pss, u0, w = problem(ins, oracle, "periodic32_3d")
    ps, method = pss[0], ins.RKMethods.RK44()
    s = len(method.b)
    field = u0.numel() * 8
    grad_rollout(ins, method, sp, ps, u0, w, 4, 4)  # handles and solver buffers exist before the measurement
    peak = {}
    for nsteps in (8, 16):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        g = grad_rollout(ins, method, sp, ps, u0, w, nsteps, 4)
        torch.cuda.synchronize()
        peak[nsteps] = (torch.cuda.max_memory_allocated() - base) / field
        del g
    print(f"peak memory in vector fields: {peak}")
    assert peak[16] - peak[8] <= 3.0, peak           # (16 - 8) / 4 = 2 more checkpoints, one field of slack
    assert peak[16] <= 4 + 4 + (2 * s + 3) + 1, peak  # checkpoints, chunk states, the work arrays of the reverse step, the cotangent


# ------------------------------------------------------------------------------------ 6. refusals
def test_refusals(ins):
    n = 16
    x = (np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1))
    method = ins.RKMethods.RK44()
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    lid = (ins.DirichletBC(), ins.DirichletBC(lambda a, x, y, t: (1.0 + 0 * x) if a == 0 else 0 * x))
    setups = [
        ins.Setup(x=x, Re=100.0, closure_model=lambda u, θ: θ * u),
        ins.Setup(x=x, Re=100.0, temperature=ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=(per, per), gdir=1)),
        ins.Setup(x=x, Re=100.0, boundary_conditions=(per, lid)),
        ins.Setup(x=x, Re=100.0, bodyforce=lambda a, x, y, t: np.sin(t) + 0 * x + 0 * y, issteadybodyforce=False),
    ]
    for sp in setups:
        ps = ins.default_psolver(sp)
        u = ins.vectorfield(sp).requires_grad_(True)
        with pytest.raises(NotImplementedError, match=r"use ad\.timestep "):
            ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u), DT, 2)


# ------------------------------------------------------------------------------------ 8. fused against two-launch reverse stages
@pytest.mark.parametrize("name,mname", [("mixed", "RK44"), ("periodic32_3d", "RK44"), ("periodic32_2d", "DOPRI6")])
def test_fused_and_two_launch_reverse_stages_agree(ins, oracle, name, mname):
    """INS_ADJ_STAGE_FUSED=1 against the default.  `mixed` runs the generic gather kernel, the uniform periodic 3-D box the tiled one; DOPRI6 has reverse
    stages with five and six terms, which keep the two launches with the switch on, beside fused ones."""
    sp, pss, u0, w = problem(ins, oracle, name)
    ps, method = pss[0], METHODS[mname](ins)
    g = {}
    for on in (0, 1):
        with ins._lib.options(INS_ADJ_STAGE_FUSED=on):
            g[on] = grad_rollout(ins, method, sp, ps, u0, w, 5, 2)
    r = rel(g[0], g[1])
    print(f"fused vs two-launch reverse stage, {name}: rel = {r:.3e}")
    assert r <= TOL, r
