"""GPU: the fused pullback of the Smagorinsky closure force (csrc/ins_smagpullback_kernels.h), `ad.smagorinsky_force` / `ad32.smagorinsky_force`, and the
closure inside the native reverse loop (`ad.timesteps(…, θ=)`, csrc/ins_rk_adjoint_loop.h).

  1. operator level, fp64: ubar and θbar of `ad.smagorinsky_force` against autograd through `ad.smagorinsky_closure(setup)(u, θ)` (both are transposes
     of one forward), on the geometries of tests/test_gpu_adjoint.py, the tile-edge grids of tests/test_gpu_adjoint_shapes.py and a periodic box with
     two interior volumes in one direction and one with a single interior volume (the source of both ghosts).  Bound: BOUND below.
  2. a field that is zero on a patch; two calls bitwise equal; accumulate; thetabar = NULL; the C-level refusals.
  3. Float32: e_new <= MARGIN e_composed against the fp64 pullback of the widened inputs.
  4. rollouts: gradients with respect to u0 and θ of 5 RK steps against 5 unrolled `ad.timestep` calls with `ad.smagorinsky_closure`, at TOL; the
     forward bitwise the native loop; a central difference in θ; a float θ; only θ requiring grad; one solver with and without θ.
"""
import ctypes as C

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_adjoint import GEOMS, TOL, _u0, mirror, nrm, rand, solvers
from tests.test_gpu_adjoint32 import MARGIN
from tests.test_gpu_adjoint_shapes import BOXES, GRIDS, aniso_box
from tests.test_gpu_ad_timesteps import DT, METHODS, loss, rel
from tests.test_gpu_stencil_tiles import make_setup

pytestmark = pytest.mark.gpu

THETA = 0.17
# 10 x the largest relative max-norm error observed over the cases of item 1 (7.03e-15, θbar on periodic32_3d), capped at TOL
BOUND = min(10 * 7.03e-15, TOL)


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


_cache = {}


def setup_of(ins, o, name):
    if name not in _cache:
        if name in GEOMS:
            sp = mirror(ins, GEOMS[name](o), o)
        elif name in GRIDS:
            sp = mirror(ins, make_setup(o, *GRIDS[name]), o)
        elif name in BOXES:
            sp = aniso_box(ins, o, BOXES[name])[1]
        elif name == "thin_periodic":  # two interior volumes in y: each is the source of one ghost of that direction and the neighbour of the other
            sp = ins.Setup(x=(np.linspace(0.0, 1.0, 10), np.linspace(0.0, 0.3, 3), np.linspace(0.0, 0.7, 6)), Re=1000.0)
        elif name == "one_periodic":  # one interior volume in y: it is the source of BOTH ghosts of that direction (three images in the product set)
            sp = ins.Setup(x=(np.linspace(0.0, 1.0, 10), np.linspace(0.0, 0.3, 2), np.linspace(0.0, 0.7, 6)), Re=1000.0)
        _cache[name] = sp
    return _cache[name]


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def both_pullbacks(ins, ad, sp, u, sbar, dtype):
    """((ubar, θbar) of ad.smagorinsky_force, (ubar, θbar) through ad.smagorinsky_closure)"""
    import torch

    out = []
    for f in (lambda uu, th: ad.smagorinsky_force(uu, th, sp), ad.smagorinsky_closure(sp)):
        uu = u.clone().requires_grad_(True)
        th = torch.tensor(THETA, dtype=dtype, device=sp.device, requires_grad=True)
        s = f(uu, th)
        out.append(torch.autograd.grad(s, (uu, th), sbar) + (s.detach(),))
    return out


OPERATOR_CASES = ["periodic32_2d", "periodic32_3d", "mixed", "box_symmetric", "box_pressure", "box_dirichlet", "setup3d", "mixed3d", "mixed2d", "b_63x37x4",
                  "thin_periodic", "one_periodic"]


@pytest.mark.parametrize("name", OPERATOR_CASES)
def test_pullback_matches_the_composed_closure(ins, oracle, name):
    """Observed relative max-norm errors (ubar, θbar) on an MI355X, each held to BOUND:
      periodic32_2d 2.63e-16, 1.71e-16   periodic32_3d 3.34e-16, 7.03e-15   mixed 4.77e-16, 6.57e-16        box_symmetric 2.77e-16, 0
      box_pressure 1.99e-16, 2.77e-16    box_dirichlet 2.75e-16, 0          setup3d 1.24e-16, 1.47e-15      mixed3d 3.08e-16, 3.51e-16
      mixed2d 1.43e-16, 3.26e-16         b_63x37x4 7.40e-16, 5.45e-16       thin_periodic 2.86e-16, 0       one_periodic 3.33e-16, 3.43e-16
    (the forward of the one native call agrees with the composed forward to <= 2.5e-16 on the degrees of freedom)."""
    import torch

    sp = setup_of(ins, oracle, name)
    u = ins.apply_bc_u(rand(ins, sp, True, 11), 0.0, sp)
    sbar = rand(ins, sp, True, 12)
    (ub, tb, s), (ub_ref, tb_ref, s_ref) = both_pullbacks(ins, ins.ad, sp, u, sbar, torch.float64)
    eu, et = relmax(ub, ub_ref), abs(float(tb - tb_ref)) / abs(float(tb_ref))
    dof = s_ref != 0
    print(f"{name}: forward {relmax(s[dof], s_ref[dof]):.2e}  ubar {eu:.2e}  thetabar {et:.2e}")
    assert float(ub_ref.abs().max()) > 0 and float(tb_ref) != 0
    assert eu <= BOUND and et <= BOUND


def test_zero_patch_is_finite(ins, oracle):
    """|S| = 0 on a patch of 6 x 6 x 6 volumes: the contribution there is defined as zero in the fused pullback and in the composed path
    (`_autodiff_core.smagorinsky_closure` masks sqrt(2 S:S) where S:S = 0), so both are finite everywhere and equal.  Measured on an MI355X, with
    the composed path restricted to its finite entries before it masked (it gave NaN at 480 of 117912): ubar 2.41e-16, θbar 2.31e-16."""
    import torch

    sp = setup_of(ins, oracle, "periodic32_3d")
    u = rand(ins, sp, True, 13)
    u[8:14, 8:14, 8:14, :] = 0.0
    u = ins.apply_bc_u(u, 0.0, sp)
    sbar = rand(ins, sp, True, 14)
    (ub, tb, _), (ub_ref, tb_ref, _) = both_pullbacks(ins, ins.ad, sp, u, sbar, torch.float64)
    assert bool(torch.isfinite(ub).all()) and bool(torch.isfinite(tb))
    ok = torch.isfinite(ub_ref)
    print(f"zero patch: composed path finite at {int(ok.sum())} of {ok.numel()} entries, θbar_ref {float(tb_ref)}")
    print(f"zero patch: where it is finite ubar {relmax(ub[ok], ub_ref[ok]):.2e}  thetabar {abs(float(tb - tb_ref)) / abs(float(tb_ref)):.2e}")
    assert relmax(ub[ok], ub_ref[ok]) <= BOUND and abs(float(tb - tb_ref)) <= BOUND * abs(float(tb_ref))
    assert bool(ok.all()) and bool(torch.isfinite(tb_ref)), "the composed path is not finite on the patch"
    assert relmax(ub, ub_ref) <= BOUND


@pytest.mark.parametrize("name", ["periodic32_3d", "mixed", "periodic32_2d"])
def test_bitwise_accumulate_null(ins, oracle, name):
    import torch

    sp = setup_of(ins, oracle, name)
    O = ins.operators
    u = ins.apply_bc_u(rand(ins, sp, True, 11), 0.0, sp)
    sbar, prev = rand(ins, sp, True, 12), rand(ins, sp, True, 15)
    runs = []
    for _ in range(2):
        tb = torch.zeros((), dtype=torch.float64, device=sp.device)
        runs.append(O.smagorinsky_force_pullback_(ins.vectorfield(sp), tb, sbar, u, THETA, sp))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    acc, _ = O.smagorinsky_force_pullback_(prev.clone(), None, sbar, u, THETA, sp, accumulate=True)  # thetabar = NULL is accepted
    assert nrm(acc - (prev + runs[0][0])) <= 4 * np.finfo(np.float64).eps * (nrm(prev) + nrm(runs[0][0]))
    none, _ = O.smagorinsky_force_pullback_(ins.vectorfield(sp), None, sbar, u, THETA, sp)
    assert torch.equal(none, runs[0][0])
    # θbar accumulates into the caller's double
    tb = torch.full((), 2.5, dtype=torch.float64, device=sp.device)
    O.smagorinsky_force_pullback_(ins.vectorfield(sp), tb, sbar, u, THETA, sp)
    assert abs(float(tb) - 2.5 - float(runs[0][1])) <= 4 * np.finfo(np.float64).eps * (2.5 + abs(float(runs[0][1])))


def test_c_level_refusals(ins, oracle):
    import torch

    sp = setup_of(ins, oracle, "periodic32_2d")
    lib = ins._lib.load()
    u, sbar = rand(ins, sp, True, 1), rand(ins, sp, True, 2)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.ins_smagorinsky_force_pullback_f64(sp.handle, THETA, p(u), p(sbar), p(u), 0, None, sp.stream) == -1
    assert lib.ins_smagorinsky_force_pullback_f64(sp.handle, THETA, p(u), p(sbar), p(sbar), 0, None, sp.stream) == -1
    u32 = u.float()
    assert lib.ins_smagorinsky_force_pullback_f32(sp.handle, THETA, p(u32), p(u32), p(u32), 0, None, sp.stream) == -1
    ps = ins.psolver_spectral(sp)
    adj = ins.ad._step_adjoint(ins.RKMethods.RK44(), sp, ps)
    assert lib.ins_rk_adjoint_set_closure(adj._handle, 2, THETA, None) == -1
    assert lib.ins_rk_adjoint_set_closure(adj._handle, 0, 0.0, None) == 0
    torch.cuda.synchronize()


def test_slab_grid_is_unsupported(ins):
    import torch

    n = 8
    x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
    bcs = ((ins.PeriodicBC(), ins.PeriodicBC()),) * 2 + ((ins.HaloBC(), ins.HaloBC()),)
    sp = ins.Setup(x=x, boundary_conditions=bcs, Re=1000.0)
    u = ins.vectorfield(sp)
    p = lambda t: C.c_void_p(t.data_ptr())
    lib = ins._lib.load()
    assert lib.ins_smagorinsky_force_pullback_f64(sp.handle, THETA, p(u), p(u.clone()), p(u.clone()), 0, None, sp.stream) == -4
    u32 = u.float()
    assert lib.ins_smagorinsky_force_pullback_f32(sp.handle, THETA, p(u32), p(u32.clone()), p(u32.clone()), 0, None, sp.stream) == -4


# ------------------------------------------------------------------------------------ 3. Float32
@pytest.mark.parametrize("name", ["periodic32_3d", "mixed", "periodic32_2d"])
def test_float32_pullback(ins, oracle, name):
    """No exact float reference: g64 is the fp64 pullback on the widened inputs, and the fused Float32 pullback may be at most MARGIN times as far from it
    as the composed Float32 path (`ad32.smagorinsky_closure`), for ubar and for θbar.  Observed on an MI355X (e_new, e_composed):
      periodic32_3d ubar 2.10e-07, 1.87e-07  θbar 1.03e-06, 1.77e-06     mixed ubar 2.63e-07, 1.87e-07  θbar 2.14e-07, 2.14e-07
      periodic32_2d ubar 8.47e-08, 1.05e-07  θbar 3.63e-08, 3.63e-08"""
    import torch

    sp = setup_of(ins, oracle, name)
    F = ins.f32
    u32 = F.apply_bc_u32_(F.to_f32(sp, rand(ins, sp, True, 11)), sp)
    sbar32 = F.to_f32(sp, rand(ins, sp, True, 12))
    u64, sbar64 = ins.from_numpy(sp, ins.to_numpy(u32.double())), ins.from_numpy(sp, ins.to_numpy(sbar32.double()))
    (g64, t64, _), _ = both_pullbacks(ins, ins.ad, sp, u64, sbar64, torch.float64)
    (ub, tb, _), (ub_c, tb_c, _) = both_pullbacks(ins, ins.ad32, sp, u32, sbar32, torch.float32)
    assert ub.dtype == torch.float32 and tb.dtype == torch.float32
    e_new, e_comp = relmax(ub.double(), g64), relmax(ub_c.double(), g64)
    t_new, t_comp = abs(float(tb) - float(t64)) / abs(float(t64)), abs(float(tb_c) - float(t64)) / abs(float(t64))
    print(f"{name}: ubar e_new {e_new:.2e} e_composed {e_comp:.2e}   thetabar e_new {t_new:.2e} e_composed {t_comp:.2e}")
    assert e_new <= MARGIN * e_comp
    assert t_new <= MARGIN * t_comp


# ------------------------------------------------------------------------------------ 4. rollouts
def problem(ins, oracle, name):
    key = ("problem", name)
    if key not in _cache:
        sp = mirror(ins, GEOMS[name](oracle), oracle)  # a setup of its own: closure_model is set on it
        ps = solvers(ins, sp, name)[0]
        _cache[key] = (sp, ps, _u0(ins, sp, ps, 80), rand(ins, sp, True, 81))
    return _cache[key]


def grads_rollout(ins, method, sp, ps, u0, w, nsteps, every, closure, θ=THETA, u_grad=True, θ_grad=True):
    import torch

    sp.closure_model = closure
    try:
        uu = u0.clone().requires_grad_(u_grad)
        th = torch.tensor(θ, dtype=torch.float64, device=sp.device, requires_grad=True) if θ_grad else θ
        out = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), DT, nsteps, θ=th, checkpoint_every=every).u
        wanted = ([uu] if u_grad else []) + ([th] if θ_grad else [])
        gs = list(torch.autograd.grad(loss(out, w), wanted)) if wanted else []
        return (gs.pop(0) if u_grad else None), (gs.pop(0) if θ_grad else None), out.detach()
    finally:
        sp.closure_model = None


def grads_unrolled(ins, method, sp, ps, u0, w, nsteps, key):
    import torch

    if key in _cache:
        return _cache[key]
    sp.closure_model = ins.ad.smagorinsky_closure(sp)
    try:
        uu = u0.clone().requires_grad_(True)
        th = torch.tensor(THETA, dtype=torch.float64, device=sp.device, requires_grad=True)
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu)
        for _ in range(nsteps):
            st = ins.ad.timestep(method, st, DT, th)
        _cache[key] = torch.autograd.grad(loss(st.u, w), (uu, th))
    finally:
        sp.closure_model = None
    return _cache[key]


def check_rollout(ins, oracle, name, mname, every, closure_of=None, nsteps=5):
    sp, ps, u0, w = problem(ins, oracle, name)
    method = METHODS[mname](ins)
    g_ref, t_ref = grads_unrolled(ins, method, sp, ps, u0, w, nsteps, ("unrolled", name, mname, nsteps))
    closure = (closure_of or ins.ad.smagorinsky_closure)(sp)
    g, t, _ = grads_rollout(ins, method, sp, ps, u0, w, nsteps, every, closure)
    eu, et = rel(g, g_ref), abs(float(t - t_ref)) / abs(float(t_ref))
    print(f"{name} {mname} nsteps={nsteps} every={every}: u0 {eu:.2e}  θ {et:.2e}  (θbar {float(t_ref):.6e})")
    assert float(t_ref) != 0 and eu <= TOL and et <= TOL
    return g, t


@pytest.mark.parametrize("name", ["periodic32_3d", "periodic32_2d", "mixed", "box_dirichlet"])
def test_rollout_gradients(ins, oracle, name):
    check_rollout(ins, oracle, name, "RK44", 2)


def test_rollout_with_the_fused_closure_as_model(ins, oracle):
    import torch

    g, t = check_rollout(ins, oracle, "periodic32_3d", "RK44", 2)
    g2, t2 = check_rollout(ins, oracle, "periodic32_3d", "RK44", 2, closure_of=ins.smagorinsky_closure)
    assert torch.equal(g, g2) and torch.equal(t, t2)


@pytest.mark.parametrize("mname", ["RK33C2", "DOPRI6", "LMWray3"])
def test_rollout_methods(ins, oracle, mname):
    check_rollout(ins, oracle, "periodic32_2d", mname, 2)


@pytest.mark.parametrize("nsteps,every", [(1, 1), (5, 1), (5, 5), (3, None)])
def test_rollout_chunkings(ins, oracle, nsteps, every):
    check_rollout(ins, oracle, "mixed", "RK44", every, nsteps=nsteps)


@pytest.mark.parametrize("name", ["periodic32_3d", "mixed"])
def test_forward_is_the_native_loop(ins, oracle, name):
    import torch

    sp, ps, u0, w = problem(ins, oracle, name)
    method = METHODS["RK44"](ins)
    before = u0.clone()
    _, _, out = grads_rollout(ins, method, sp, ps, u0, w, 5, 2, ins.ad.smagorinsky_closure(sp), θ_grad=False)
    assert torch.equal(u0, before)
    sp.closure_model = ins.smagorinsky_closure(sp)
    try:
        cache = ins.ode_method_cache(method, sp, ps)
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=u0.clone())
        for n in (2, 2, 1):
            st = ins.timesteps_(method, st, DT, n, θ=THETA, cache=cache)
        assert torch.equal(out, st.u), "not bitwise the native loop with the same chunking"
        with torch.no_grad():
            a = ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), DT, 5, θ=THETA, checkpoint_every=2).u
        one = ins.timesteps_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0.clone()), DT, 5, θ=THETA, cache=cache).u
        assert a.grad_fn is None and torch.equal(a, one)
        plain = ins.timesteps_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0.clone()), DT, 5, θ=0.0, cache=cache).u
        assert not torch.equal(plain, one), "the closure did not enter the forward"
    finally:
        sp.closure_model = None


def test_theta_alone(ins, oracle):
    import torch

    name = "periodic32_2d"
    sp, ps, u0, w = problem(ins, oracle, name)
    method = METHODS["RK44"](ins)
    closure = ins.ad.smagorinsky_closure(sp)
    g, t, _ = grads_rollout(ins, method, sp, ps, u0, w, 5, 2, closure)
    e = 1e-6
    Lp = float(loss(grads_rollout(ins, method, sp, ps, u0, w, 5, 2, closure, θ=THETA + e, u_grad=False, θ_grad=False)[2], w))
    Lm = float(loss(grads_rollout(ins, method, sp, ps, u0, w, 5, 2, closure, θ=THETA - e, u_grad=False, θ_grad=False)[2], w))
    fd = (Lp - Lm) / (2 * e)
    print(f"θbar {float(t):.9e}  central difference {fd:.9e}")
    assert abs(float(t) - fd) <= 1e-6 + 1e-6 * abs(fd)
    g_float, none, _ = grads_rollout(ins, method, sp, ps, u0, w, 5, 2, closure, θ_grad=False)
    assert none is None and torch.equal(g_float, g)
    _, t_only, _ = grads_rollout(ins, method, sp, ps, u0, w, 5, 2, closure, u_grad=False)
    assert torch.equal(t_only, t)


def test_one_solver_with_and_without_theta(ins, oracle):
    """A rollout with θ, then the same setup with closure_model removed on the same solver: bitwise what a fresh handle gives."""
    import torch

    from tests.test_gpu_ad_timesteps import grad_rollout

    sp, ps, u0, w = problem(ins, oracle, "mixed")
    method = METHODS["RK44"](ins)
    grads_rollout(ins, method, sp, ps, u0, w, 5, 2, ins.ad.smagorinsky_closure(sp))
    after = grad_rollout(ins, method, sp, ps, u0, w, 5, 2)
    fresh_ps = solvers(ins, sp, "mixed")[0]
    fresh = grad_rollout(ins, method, sp, fresh_ps, u0, w, 5, 2)
    assert torch.equal(after, fresh)


def test_refusals(ins, oracle):
    sp, ps, u0, w = problem(ins, oracle, "periodic32_2d")
    other = setup_of(ins, oracle, "periodic32_2d")
    method = METHODS["RK44"](ins)
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u0)
    cases = [(lambda u, θ: u, THETA), (ins.ad.smagorinsky_closure(sp), None), (None, THETA), (ins.ad.smagorinsky_closure(other), THETA),
             (ins.smagorinsky_closure(other), THETA)]
    for closure, θ in cases:
        sp.closure_model = closure
        try:
            with pytest.raises(NotImplementedError, match="timestep "):
                ins.ad.timesteps(method, st, DT, 2, θ=θ)
        finally:
            sp.closure_model = None
