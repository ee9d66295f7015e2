"""GPU: the Smagorinsky closure in the native reverse loop beyond the isothermal fp64 cases of tests/test_gpu_smag_pullback.py.

  1. Float32: `ad32.timesteps(…, θ=)` on `periodic32_3d` (spectral32) and on `mixed` (a wrapped direct solver), under the rule of
     tests/test_gpu_ad32_timesteps.py item 2: g64 is the fp64 `ad.timesteps(…, θ=)` gradient on the widened inputs, e_native the error of
     `ad32.timesteps`, e_unrolled that of 5 chained `ad32.timestep` calls with `ad32.smagorinsky_closure`; e_native <= MARGIN e_unrolled for u0 and for θ.
     Observed on an MI355X (e_native, e_unrolled): periodic32_3d u0 1.44e-07, 1.60e-07  θ 1.95e-08, 4.38e-08;  mixed u0 1.32e-07, 2.23e-07  θ 2.64e-08, 9.66e-08.
  2. with the temperature equation: the 2-D Rayleigh-Benard box of tests/test_gpu_ad_timesteps_temp.py with the closure; gradients with respect to u0,
     temp0 and θ against 5 chained `ad.timestep` calls at TOL.
  3. peak memory (the method of test_peak_memory_grows_by_the_checkpoints_only): with the closure the torch peak of forward + backward is that of the
     closure-free rollout (θbar is one double), it grows with the checkpoints only, and the device memory the first closure rollout takes outside
     torch is the closure scratch: one vector field on the handle, D·D scalar fields of ∇ubar and the workgroup partials on the grid handle (no
     `sigma` on a periodic 3-D box: the force is one kernel there).
"""
import pytest

from tests.test_gpu_ad_timesteps import DT, METHODS, rel
from tests.test_gpu_adjoint import TOL, nrm
from tests.test_gpu_adjoint32 import GEOMS, MARGIN, mirror, pair
from tests.test_gpu_adjoint32 import _u0 as _u0_pair

pytestmark = pytest.mark.gpu

THETA = 0.17
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def release_problems():
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


def loss(u, w):
    return 0.5 * (w * u.double() * u.double()).sum()


# ------------------------------------------------------------------------------------ 1. Float32
def problem32(ins, oracle, name):
    if name not in _cache:
        sp = mirror(ins, GEOMS[name](oracle), oracle)
        if name.startswith("periodic"):
            ps32, ps64 = ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)
        else:
            ps64 = ins.psolver_direct(sp)
            ps32 = ins.f32.psolver_wrap32(sp, ins.psolver_direct(sp))
        _cache[name] = (sp, ps32, ps64, _u0_pair(ins, sp, ps64, 50), pair(ins, sp, True, 52)[1].abs())
    return _cache[name]


def gradients(ins, ad, rollout, method, sp, ps, u, w, dtype, closure):
    """(∂L/∂u0 flattened in double, ∂L/∂θ as a float) of 5 steps with the closure `closure(sp)` as the setup's model"""
    import torch

    sp.closure_model = closure(sp)
    try:
        uu = u.clone().requires_grad_(True)
        th = torch.tensor(THETA, dtype=dtype, device=sp.device, requires_grad=True)
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=uu)
        if rollout:
            st = ad.timesteps(method, st, DT, 5, θ=th, checkpoint_every=2)
        else:
            for _ in range(5):
                st = ad.timestep(method, st, DT, th)
        gu, gt = torch.autograd.grad(loss(st.u, w), (uu, th))
        assert gu.dtype == dtype and gt.dtype == dtype
        return gu.detach().double().reshape(-1), float(gt)
    finally:
        sp.closure_model = None


@pytest.mark.parametrize("name", ["periodic32_3d", "mixed"])
def test_float32_rollout(ins, oracle, name):
    import torch

    sp, ps32, ps64, (u32, u64), w = problem32(ins, oracle, name)
    method = METHODS["RK44"](ins)
    g64, t64 = gradients(ins, ins.ad, True, method, sp, ps64, u64, w, torch.float64, ins.ad.smagorinsky_closure)
    gun, tun = gradients(ins, ins.ad32, False, method, sp, ps32, u32, w, torch.float32, ins.ad32.smagorinsky_closure)
    gnat, tnat = gradients(ins, ins.ad32, True, method, sp, ps32, u32, w, torch.float32, ins.ad32.smagorinsky_closure)
    e_nat, e_unr = float((gnat - g64).norm() / g64.norm()), float((gun - g64).norm() / g64.norm())
    t_nat, t_unr = abs(tnat - t64) / abs(t64), abs(tun - t64) / abs(t64)
    print(f"RATIO ad32.timesteps θ {name}: u0 e_native={e_nat:.3e} e_unrolled={e_unr:.3e}   θ e_native={t_nat:.3e} e_unrolled={t_unr:.3e} (θbar64 {t64:.6e})")
    assert float(g64.norm()) > 0 and t64 != 0 and e_unr > 0
    assert e_nat <= MARGIN * e_unr
    assert t_nat <= MARGIN * t_unr
    # the fused Float32 closure as the setup's model: the same native loops
    g2, t2 = gradients(ins, ins.ad32, True, method, sp, ps32, u32, w, torch.float32, ins.f32.smagorinsky_closure32)
    assert torch.equal(g2, gnat) and t2 == tnat


# ------------------------------------------------------------------------------------ 2. with the temperature equation
def test_rayleigh_benard_with_the_closure(ins, oracle):
    import torch

    from tests import test_gpu_ad_timesteps_temp as tt

    sp, ps, u0, t0, w, wt = tt.problem(ins, oracle, "rb2d")
    method = METHODS["RK44"](ins)
    sp.closure_model = ins.ad.smagorinsky_closure(sp)
    try:
        out = []
        for rollout in (True, False):
            uu, te = u0.clone().requires_grad_(True), t0.clone().requires_grad_(True)
            th = torch.tensor(THETA, dtype=torch.float64, device=sp.device, requires_grad=True)
            st = tt.stepper(ins, method, sp, ps, uu, te)
            if rollout:
                st = ins.ad.timesteps(method, st, DT, 5, θ=th, checkpoint_every=2)
            else:
                for _ in range(5):
                    st = ins.ad.timestep(method, st, DT, th)
            out.append(torch.autograd.grad(tt.loss(st.u, st.temp, w, wt), (uu, te, th)))
    finally:
        sp.closure_model = None
    (gu, gT, gth), (ru, rT, rth) = out
    eu, eT, eth = rel(gu, ru), rel(gT, rT), abs(float(gth - rth)) / abs(float(rth))
    print(f"rb2d with closure: u0 {eu:.2e}  temp0 {eT:.2e}  θ {eth:.2e}  (θbar {float(rth):.6e})")
    assert nrm(ru) > 0 and nrm(rT) > 0 and float(rth) != 0
    assert eu <= TOL and eT <= TOL and eth <= TOL


# ------------------------------------------------------------------------------------ 3. memory
def test_peak_memory_with_the_closure(ins, oracle):
    import torch

    from tests.test_gpu_ad_timesteps import grad_rollout
    from tests.test_gpu_ad_timesteps import problem as problem64
    from tests.test_gpu_smag_pullback import grads_rollout

    sp, pss, u0, w = problem64(ins, oracle, "periodic32_3d")
    ps, method = ins.psolver_spectral(sp), ins.RKMethods.RK44()  # a solver of its own: its reverse-step handle has never carried a closure
    s, D = len(method.b), 3
    field = u0.numel() * 8
    closure = ins.ad.smagorinsky_closure(sp)
    grad_rollout(ins, method, sp, ps, u0, w, 4, 4)  # handles and solver buffers exist before the measurement

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        g = fn()
        torch.cuda.synchronize()
        p = (torch.cuda.max_memory_allocated() - base) / field
        del g
        return p

    try:
        sp.closure_model = closure
        with torch.no_grad():  # the forward loop's own closure scratch (the native cache's, there before this change) exists before the measurement
            ins.ad.timesteps(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), DT, 2, θ=THETA)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        first = peak_of(lambda: grads_rollout(ins, method, sp, ps, u0, w, 4, 4, closure))  # allocates the closure scratch, outside torch
        torch.cuda.synchronize()
        scratch = (free0 - torch.cuda.mem_get_info()[0]) / field
        plain = {n: peak_of(lambda: grad_rollout(ins, method, sp, ps, u0, w, n, 4)) for n in (8, 16)}
        with_m = {n: peak_of(lambda: grads_rollout(ins, method, sp, ps, u0, w, n, 4, closure)) for n in (8, 16)}
    finally:
        sp.closure_model = None
    print(f"peak torch memory in vector fields: plain {plain}, with closure {with_m} (first {first:.2f}); device memory taken outside torch by the first "
          f"closure rollout: {scratch:.2f} fields")
    # torch side: θ and θbar are scalars (torch rounds an allocation up to 512 bytes; a quarter field of slack)
    for n in (8, 16):
        assert with_m[n] <= plain[n] + 0.25, (plain, with_m)
    assert with_m[16] - with_m[8] <= 3.0, with_m           # (16 - 8) / 4 = 2 more checkpoints, one field of slack: nothing grows with nsteps · nstage
    assert with_m[16] <= 4 + 4 + (2 * s + 3) + 1, with_m    # the bound of the closure-free rollout
    # library side: one vector field (closure force) + D·D scalars = D vector fields (∇ubar) + the partials (a few KB); three device allocations, each
    # rounded up by the runtime to at most 2 MiB
    assert scratch <= 1 + D + 3 * (2 << 20) / field, scratch
