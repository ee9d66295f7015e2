"""GPU: `ad.timesteps` with the temperature equation and the native coupled step pullback ins_rk_step_pullback_ext_f64 (csrc/ins_rk_adjoint_loop.h).

  1. forward: (u, temp) bitwise `timesteps_` with the same chunking; the inputs are untouched; without grad nothing is saved, same numbers;
  2. gradient of a weighted quadratic loss in both outputs with respect to u0 and temp0 against 5 chained `ad.timestep` calls,
     ||g - g_ref|| <= TOL ||g_ref|| for each of the two, TOL = 1e-12 of tests/test_gpu_adjoint.py (the same kernels, another summation order);
  3. 32 random rows of the dense transpose of one coupled RK44 step against central differences of the native step ins_rk_step_ext_f64;
  4. Taylor test through 20 RK44 steps on the 2-D Rayleigh-Benard box: the central remainder falls by 8 per halving;
  5. peak memory of backward grows with the checkpoints only ((D+1)/D fields per state);
  6. only one of u0, temp0 requires grad: its gradient is bitwise the one of the run in which both do.

Temperature sides: every kind of tests/test_gpu_temp_adjoint.KINDS.  On a geometry with walls the kind "function" is callable Dirichlet data, which
`ad.timesteps` refuses by design (the host has to evaluate it between the stages): there the test asserts that refusal; on periodic boxes every kind
is periodic and runs.
"""
import numpy as np
import pytest

from tests.test_gpu_ad_timesteps import DT, METHODS, rel
from tests.test_gpu_adjoint import TOL, _u0, dot, nrm, rand, relmax, solvers
from tests.test_gpu_temp_adjoint import KINDS, _rb_setup, _rb_temp0, gdirs, with_temperature

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_problems():
    """The problems are built once per module and released with it: solvers, reverse-step handles and native caches do not outlive the file."""
    import gc

    yield
    _cache.clear()
    gc.collect()


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def periodic3d(ins, gdir, diss):
    """8^3 periodic box: the smallest 3-D box the spectral solver and the tiled kernels take."""
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, dodissipation=diss, gdir=gdir, boundary_conditions=(per, per, per))
    return ins.Setup(x=tuple(np.linspace(0.0, 1.0, 9) for _ in range(3)), Re=1000.0, temperature=T)


def problem(ins, oracle, name, kind="dirichlet", gdir=1, diss=True):
    """(setup, solver, u0, temp0, w, wtemp), built once per module"""
    key = (name, kind, gdir, diss)
    if key not in _cache:
        if name == "periodic3d":
            sp = periodic3d(ins, gdir, diss)
        elif name == "rb2d":
            sp = _rb_setup(ins, 16)
        else:
            _, sp = with_temperature(ins, oracle, name, kind, gdir, dodissipation=diss)
        ps = ins.default_psolver(sp) if name in ("periodic3d", "rb2d") else solvers(ins, sp, name)[0]  # the 7 x 7 periodic box: direct
        u0 = _u0(ins, sp, ps, 80)
        t0 = _rb_temp0(ins, sp) if name == "rb2d" else ins.apply_bc_temp(0.5 + 0.1 * rand(ins, sp, False, 41), 0.0, sp)
        _cache[key] = (sp, ps, u0, t0, rand(ins, sp, True, 81), rand(ins, sp, False, 82))
    return _cache[key]


def loss(u, temp, w, wt):
    return 0.5 * (w * u * u).sum() + 0.5 * (wt * temp * temp).sum()


def stepper(ins, method, sp, ps, u, temp):
    return ins.create_stepper(method, setup=sp, psolver=ps, u=u, temp=temp)


def grad_rollout(ins, method, prob, nsteps, every, req=(True, True)):
    import torch

    sp, ps, u0, t0, w, wt = prob
    uu, tt = u0.clone().requires_grad_(req[0]), t0.clone().requires_grad_(req[1])
    out = ins.ad.timesteps(method, stepper(ins, method, sp, ps, uu, tt), DT, nsteps, checkpoint_every=every)
    return torch.autograd.grad(loss(out.u, out.temp, w, wt), [x for x, r in zip((uu, tt), req) if r])


def grad_unrolled(ins, method, prob, nsteps, key):
    """the reference: nsteps calls of ad.timestep through torch autograd, computed once per key"""
    import torch

    if key in _cache:
        return _cache[key]
    sp, ps, u0, t0, w, wt = prob
    uu, tt = u0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    st = stepper(ins, method, sp, ps, uu, tt)
    for _ in range(nsteps):
        st = ins.ad.timestep(method, st, DT)
    _cache[key] = torch.autograd.grad(loss(st.u, st.temp, w, wt), (uu, tt))
    return _cache[key]


# ------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name,mname", [("periodic32_2d", "RK44"), ("mixed", "RK44"), ("box_dirichlet", "LMWray3")])
def test_forward_is_the_native_loop(ins, oracle, name, mname):
    import torch

    sp, ps, u0, t0, _, _ = problem(ins, oracle, name)
    method = METHODS[mname](ins)
    ubefore, tbefore = u0.clone(), t0.clone()
    uu, tt = u0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    got = ins.ad.timesteps(method, stepper(ins, method, sp, ps, uu, tt), DT, 5, checkpoint_every=2)
    assert got.u.grad_fn is not None and got.temp.grad_fn is not None and got.n == 5 and abs(got.t - 5 * DT) < 1e-15
    assert torch.equal(uu.detach(), ubefore) and torch.equal(tt.detach(), tbefore), "an input was changed"
    cache = ins.ode_method_cache(method, sp, ps)
    st = stepper(ins, method, sp, ps, u0.clone(), t0.clone())
    for n in (2, 2, 1):
        st = ins.timesteps_(method, st, DT, n, cache=cache)
    assert torch.equal(got.u.detach(), st.u) and torch.equal(got.temp.detach(), st.temp), "not bitwise the native loop with the same chunking"
    with torch.no_grad():
        a = ins.ad.timesteps(method, stepper(ins, method, sp, ps, uu, tt), DT, 5, checkpoint_every=2)
    b = ins.ad.timesteps(method, stepper(ins, method, sp, ps, u0, t0), DT, 5, checkpoint_every=2)
    for x in (a, b):
        assert x.u.grad_fn is None and x.temp.grad_fn is None and not x.u.requires_grad and not x.temp.requires_grad
        assert torch.equal(x.u, st.u) and torch.equal(x.temp, st.temp)


# ------------------------------------------------------------------------------------ 2. gradient against the unrolled path
def check_gradient(ins, oracle, name, mname, nsteps, every, kind="dirichlet", gdir=1, diss=True):
    prob = problem(ins, oracle, name, kind, gdir, diss)
    method = METHODS[mname](ins)
    ref = grad_unrolled(ins, method, prob, nsteps, key=("ref", name, kind, gdir, diss, mname, nsteps))
    g = grad_rollout(ins, method, prob, nsteps, every)
    ru, rt = rel(g[0], ref[0]), rel(g[1], ref[1])
    print(f"ad.timesteps vs unrolled: {name} {kind} gdir={gdir} diss={diss} {mname} nsteps={nsteps} every={every}: rel u0 = {ru:.3e}, temp0 = {rt:.3e}")
    assert nrm(ref[0]) > 0 and nrm(ref[1]) > 0
    assert ru <= TOL and rt <= TOL, (name, kind, gdir, diss, mname, nsteps, every, ru, rt)


def _geom_cases(oracle_names=("box_periodic", "box_dirichlet", "mixed")):
    return [(n, k) for n in oracle_names for k in KINDS] + [("periodic3d", "any")]  # all sides periodic: one kind covers the box


@pytest.mark.parametrize("diss", [True, False])
@pytest.mark.parametrize("name,kind", _geom_cases())
def test_gradient_matches_unrolled_geometries(ins, oracle, name, kind, diss):
    """RK44, five steps in chunks of two (a ragged last chunk); every kind of temperature side, every gravity direction, dissipation on and off."""
    dirs = [1, 2] if name == "periodic3d" else gdirs(oracle, name)
    for gdir in dirs:
        if kind == "function" and name in ("box_dirichlet", "mixed"):
            _, sp = with_temperature(ins, oracle, name, kind, gdir, dodissipation=diss)
            ps = ins.default_psolver(sp)
            method = METHODS["RK44"](ins)
            u, t = ins.vectorfield(sp).requires_grad_(True), ins.scalarfield(sp)
            with pytest.raises(NotImplementedError, match=r"use ad\.timestep "):
                ins.ad.timesteps(method, stepper(ins, method, sp, ps, u, t), DT, 5, checkpoint_every=2)
            continue
        check_gradient(ins, oracle, name, "RK44", 5, 2, kind, gdir, diss)


@pytest.mark.parametrize("mname", ["RK33C2", "LMWray3", "DOPRI6"])
def test_gradient_matches_unrolled_methods(ins, oracle, mname):
    check_gradient(ins, oracle, "box_dirichlet", mname, 5, 2)


@pytest.mark.parametrize("nsteps,every", [(1, 1), (5, 1), (5, 2), (5, 5), (3, None)])
def test_gradient_matches_unrolled_chunkings(ins, oracle, nsteps, every):
    check_gradient(ins, oracle, "mixed", "RK44", nsteps, every, "any")


# ------------------------------------------------------------------------------------ 3. dense transpose of one coupled step
def test_step_pullback_rows_match_central_differences(ins, oracle):
    """Rows of the coupled step's Jacobian on the smallest box, by unit cotangents in u or in temp through ins_rk_step_pullback_ext_f64, against central
    differences of the native step ins_rk_step_ext_f64; Δt = 1e-5 and h = 2^-7 as in tests/test_gpu_ad_timesteps.py item 3, and its acceptance rule."""
    import torch

    from ins_amd import _lib

    sp, ps, u0, t0, _, _ = problem(ins, oracle, "box_dirichlet")
    method = ins.RKMethods.RK44()
    dt, h = 1e-5, 2.0**-7
    adj = ins.ad._step_adjoint(method, sp, ps)
    cache = ins.ode_method_cache(method, sp, ps)
    N, D = tuple(sp.grid.N), sp.grid.dimension
    ushape = N + (D,)
    nu, nt = int(np.prod(ushape)), int(np.prod(N))
    n = nu + nt

    def split(x):
        return x[:nu].reshape(ushape, order="F"), x[nu:].reshape(N, order="F")

    def step(x):
        a, b = split(x)
        st = ins.timestep_(method, stepper(ins, method, sp, ps, ins.from_numpy(sp, a), ins.from_numpy(sp, b)), dt, cache=cache)
        return np.concatenate([ins.to_numpy(st.u).reshape(-1, order="F"), ins.to_numpy(st.temp).reshape(-1, order="F")])

    base = np.concatenate([ins.to_numpy(u0).reshape(-1, order="F"), ins.to_numpy(t0).reshape(-1, order="F")])
    J = np.empty((n, n))
    e = np.zeros(n)
    for m in range(n):
        e[m] = h
        J[:, m] = (step(base + e) - step(base - e)) / (2 * h)
        e[m] = 0.0
    rows = np.sort(np.random.default_rng(7).choice(n, size=32, replace=False))
    assert (rows < nu).any() and (rows >= nu).any()
    got = np.empty((len(rows), n))
    for r, k in enumerate(rows):
        cot = np.zeros(n)
        cot[k] = 1.0
        a, b = split(cot)
        ubar, tbar = ins.from_numpy(sp, a), ins.from_numpy(sp, b)
        adj.step_pullback_(ubar, u0, dt, tbar, t0)
        got[r] = np.concatenate([ins.to_numpy(ubar).reshape(-1, order="F"), ins.to_numpy(tbar).reshape(-1, order="F")])
    err = relmax(got, J[rows])
    print(f"coupled step pullback rows vs central differences: relmax = {err:.3e}")
    assert np.max(np.abs(J[rows])) > 0.5 and err <= TOL, err
    # aliased and missing arguments are refused
    lib = _lib.load()
    u, t, ub, tb = u0.clone(), t0.clone(), u0.clone(), t0.clone()
    args = lambda us, ts, ubar, tbar: (adj._handle, 1.0 / sp.Re, us, ts, None, dt, ubar, tbar, sp.stream)  # noqa: E731
    pu, pt, pub, ptb = sp.ptr(u, True), sp.ptr(t, False), sp.ptr(ub, True), sp.ptr(tb, False)
    for bad in (args(pu, pt, pu, ptb), args(pu, pt, pub, pt), args(pu, pt, pub, pub)):
        assert lib.ins_rk_step_pullback_ext_f64(*bad) == -1 and b"alias" in lib.ins_last_error()
    assert lib.ins_rk_step_pullback_ext_f64(*args(pu, None, pub, ptb)) == -1 and lib.ins_rk_step_pullback_ext_f64(*args(pu, pt, pub, None)) == -1
    fresh = ins.ad._OPS.rk_adjoint_create(method, sp, ps)
    assert lib.ins_rk_step_pullback_ext_f64(fresh, 1.0 / sp.Re, pu, pt, None, dt, pub, ptb, sp.stream) == -1  # no descriptor set
    assert lib.ins_rk_adjoint_destroy(fresh) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ 4. Taylor test
def test_taylor_through_20_steps(ins, oracle):
    """|L(x + hv) - L(x - hv) - 2h <g, v>| with x = (u0, temp0) is the cubic remainder: it falls by 8 per halving of h over h = 1e-2 / 2^k, k = 0..3,
    the range and the acceptance (8 +- 1) of tests/test_gpu_ad_timesteps.py item 4, on the 16 x 16 Rayleigh-Benard box."""
    import torch

    sp, ps, u0, t0, w, wt = problem(ins, oracle, "rb2d")
    method = ins.RKMethods.RK44()
    vu = _u0(ins, sp, ps, 84)
    vu = vu * (nrm(u0) / nrm(vu))
    vt = ins.apply_bc_temp(rand(ins, sp, False, 85), 0.0, sp) - ins.apply_bc_temp(ins.scalarfield(sp), 0.0, sp)
    vt = vt * (nrm(t0) / nrm(vt))
    uu, tt = u0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
    out = ins.ad.timesteps(method, stepper(ins, method, sp, ps, uu, tt), DT, 20)
    gu, gt = torch.autograd.grad(loss(out.u, out.temp, w, wt), (uu, tt))
    dJ = dot(gu, vu) + dot(gt, vt)

    def L(e):
        with torch.no_grad():
            o = ins.ad.timesteps(method, stepper(ins, method, sp, ps, u0 + e * vu, t0 + e * vt), DT, 20)
            return float(loss(o.u, o.temp, w, wt))

    hs = [1e-2 / 2**k for k in range(4)]
    r = [abs(L(h) - L(-h) - 2 * h * dJ) for h in hs]
    ratios = [r[k] / r[k + 1] for k in range(3)]
    print(f"Taylor remainders {r}, ratios {ratios}")
    assert all(abs(x - 8.0) <= 1.0 for x in ratios), (r, ratios)


# ------------------------------------------------------------------------------------ 5. memory
def test_peak_memory_grows_by_the_checkpoints_only(ins, oracle):
    """The bound of tests/test_gpu_ad_timesteps.py item 5 with (D+1)/D vector fields per state."""
    import torch

    prob = problem(ins, oracle, "periodic32_2d")
    sp, u0 = prob[0], prob[2]
    method = ins.RKMethods.RK44()
    s, D = len(method.b), sp.grid.dimension
    per_state = (D + 1) / D
    field = u0.numel() * 8
    grad_rollout(ins, method, prob, 4, 4)  # handles and solver buffers exist before the measurement
    peak = {}
    for nsteps in (8, 16):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        g = grad_rollout(ins, method, prob, nsteps, 4)
        torch.cuda.synchronize()
        peak[nsteps] = (torch.cuda.max_memory_allocated() - base) / field
        del g
    print(f"peak memory in vector fields: {peak}")
    assert peak[16] - peak[8] <= 3.0 * per_state, peak
    assert peak[16] <= (4 + 4 + (2 * s + 3) + 1) * per_state, peak


# ------------------------------------------------------------------------------------ 6. one input requires grad
@pytest.mark.parametrize("which", [0, 1])
def test_one_input_requires_grad(ins, oracle, which):
    import torch

    prob = problem(ins, oracle, "mixed")
    method = ins.RKMethods.RK44()
    both = grad_rollout(ins, method, prob, 5, 2)
    (one,) = grad_rollout(ins, method, prob, 5, 2, req=tuple(q == which for q in range(2)))
    assert torch.equal(one, both[which])
