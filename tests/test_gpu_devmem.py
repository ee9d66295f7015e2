"""GPU: no handle of libinship leaves device or pinned-host memory behind.  Every buffer of every handle is a DevBuf / HostPinned member
(csrc/ins_devbuf.h), and `ins_dbg_dev_live` counts what the allocation seam (csrc/ins_devmem.hip) has handed out and not taken back.  Each block below
creates one family of handles on the smallest box its path accepts (the shapes of tools/rk_paths_hash.py and tests/test_gpu_parity.py), uses it once and
drops it; after each block, and after all of them, the count of buffers and of bytes is back where it started.  No allocation failure is provoked."""
import ctypes as C
import gc

import numpy as np
import pytest

from tests import fixtures as fx
from tests import tensorbasis_ref as tr

pytestmark = pytest.mark.gpu
DT = 2e-3


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def live(ins):
    import torch

    torch.cuda.synchronize()
    gc.collect()
    n, b = C.c_int64(-1), C.c_int64(-1)
    ins._lib.load().ins_dbg_dev_live(C.byref(n), C.byref(b))
    return n.value, b.value


def exact(n):
    """uniform spacings that are exact binary fractions"""
    return tuple(np.arange(ni + 1) / 2.0 ** int(np.ceil(np.log2(ni))) for ni in n)


def walls(ins):
    """the small wall-bounded 3-D box of tools/rk_paths_hash.py: stretched x, cosine y with a moving lid, periodic z"""
    P, Dn = ins.PeriodicBC, ins.DirichletBC
    t = np.linspace(0.0, 1.0, 25)
    x = (1 + np.tanh(1.2 * (2 * t - 1)) / np.tanh(1.2)) / 2
    y = (1 - np.cos(np.pi * np.arange(11) / 10)) / 2
    return (x, y, np.linspace(-0.2, 0.2, 9)), ((Dn(), Dn()), (Dn(), Dn((1.0, 0.2, 0.0))), (P(), P()))


def start(ins, sp, ps, seed=11):
    D = sp.grid.dimension
    u = ins.apply_bc_u(ins.from_numpy(sp, 0.1 * fx.randn_field(tuple(sp.grid.N) + (D,), seed)), 0.0, sp)
    return ins.apply_bc_u(ins.project(u, sp, ps), 0.0, sp)


def periodic_f64(ins, n):
    """spectral solver, a native 3-step call, ad.timesteps forward + backward, a spectrum observer"""
    sp = ins.Setup(x=exact(n), Re=200.0)
    ps = ins.psolver_spectral(sp)
    u0 = start(ins, sp, ps)
    m = ins.RKMethods.RK44()
    cache = ins.ode_method_cache(m, sp, ps)
    st = ins.timesteps_(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u0.clone()), DT, 3, cache=cache)
    assert bool(st.u.isfinite().all())
    u = u0.clone().requires_grad_(True)
    out = ins.ad.timesteps(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u), DT, 3)
    (out.u * out.u).sum().backward()
    assert bool(u.grad.isfinite().all())
    state = ins.Observable(dict(u=st.u, t=0.0))
    spec = ins.observespectrum(state, setup=sp)
    assert np.all(np.isfinite(spec["ehat"].value))
    return live(ins)[0]  # while everything is alive


def walls_f64(ins):
    """direct solver + one step (tiled loop: ub copies of the caller's field), CG solver + one solve"""
    x, bc = walls(ins)
    sp = ins.Setup(x=x, Re=200.0, boundary_conditions=bc)
    ps = ins.psolver_direct(sp)
    u0 = start(ins, sp, ps)
    m = ins.RKMethods.RK44()
    dt = min(DT, 0.5 * ins.get_cfl_timestep_(None, u0, sp))
    st = ins.timestep_(m, ins.create_stepper(m, setup=sp, psolver=ps, u=u0.clone()), dt, cache=ins.ode_method_cache(m, sp, ps))
    assert bool(st.u.isfinite().all())
    cg = ins.psolver_cg(sp)
    f = ins.scalewithvolume(ins.divergence(ins.apply_bc_u(ins.from_numpy(sp, fx.randn_field(tuple(sp.grid.N) + (3,), 8)), 0.0, sp), sp), sp)
    assert bool(ins.poisson(cg, f).isfinite().all())
    return live(ins)[0]


def family_f32(ins):
    """ERKCache32 on 16³; the temperature equation with the Smagorinsky closure on the Rayleigh-Bénard-style walls box; an ad32 rollout on 16³"""
    f32 = ins.f32
    sp = ins.Setup(x=exact((16, 16, 16)), Re=500.0)
    u0 = start(ins, sp, ins.default_psolver(sp), seed=5)
    ps = f32.default_psolver32(sp)
    m = ins.RKMethods.RK44()
    cache = f32.ERKCache32(m, sp, ps)
    u = f32.to_f32(sp, ins.to_numpy(u0))
    f32.timesteps32_(cache, u, DT, 3)
    assert bool(u.isfinite().all())
    ua = f32.to_f32(sp, ins.to_numpy(u0)).requires_grad_(True)
    out = ins.ad32.timesteps(m, ins.create_stepper(m, setup=sp, psolver=ps, u=ua), DT, 3)
    (out.u * out.u).sum().backward()
    assert bool(ua.grad.isfinite().all())
    # hot bottom, cold top, symmetric x sides, periodic z
    x, bc = walls(ins)
    tbc = ((ins.SymmetricBC(), ins.SymmetricBC()), (ins.DirichletBC(1.0), ins.DirichletBC(0.0)), (ins.PeriodicBC(), ins.PeriodicBC()))
    T = ins.temperature_equation(Pr=0.71, Ra=1e6, Ge=0.1, boundary_conditions=tbc, gdir=1, dodissipation=True)
    rb = ins.Setup(x=x, boundary_conditions=bc, temperature=T)
    rb.closure_model = f32.smagorinsky_closure32(rb)
    ps64 = ins.psolver_direct(rb)
    w0 = start(ins, rb, ps64, seed=5)
    dt = min(DT, 0.5 * ins.get_cfl_timestep_(None, w0, rb))
    psw = f32.psolver_wrap32(rb, ps64)
    cw = f32.ERKCache32(m, rb, psw)
    w = f32.to_f32(rb, ins.to_numpy(w0))
    t = f32.apply_bc_temp32_(f32.to_f32(rb, 0.5 + 0.1 * fx.randn_field(tuple(rb.grid.N), 4)), rb)
    f32.timesteps32_(cw, w, dt, 3, temp=t, θ=0.17)
    assert bool(w.isfinite().all()) and bool(t.isfinite().all())
    return live(ins)[0]


def ensemble(ins):
    sp = ins.Setup(x=exact((16, 16)), Re=500.0)
    ps = ins.psolver_spectral(sp)
    U = ins.vectorfields(sp, 2)
    for b in range(2):
        U[b].copy_(start(ins, sp, ps, seed=20 + b))
    ins.timesteps_ensemble_(ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, 2), U, 0.0, DT, 2)
    assert bool(U.isfinite().all())
    return live(ins)[0]


def tensor_closure(ins):
    """the fused pullback takes the grid's ∇ubar scratch on first use"""
    sp = ins.Setup(x=exact((16, 16)), Re=500.0)
    nb, _, ns = tr.sizes(2)
    N = tuple(sp.grid.N)
    u, a, taubar = (ins.from_numpy(sp, fx.randn_field(N + (k,), 30 + k)) for k in (2, nb, ns))
    before = live(ins)[0]
    ub = ins.tensorclosure_pullback_(ins.vectorfield(sp), ins.from_numpy(sp, np.zeros(N + (nb,), order="F")), taubar, None, u, a, sp)
    assert bool(ub.isfinite().all())
    now = live(ins)[0]
    assert now == before + 1  # the scratch, and nothing else
    return now


BLOCKS = [("periodic 16^3", lambda ins: periodic_f64(ins, (16, 16, 16))), ("periodic 64x32", lambda ins: periodic_f64(ins, (64, 32))), ("walls", walls_f64),
          ("float32 family", family_f32), ("ensemble", ensemble), ("tensor closure", tensor_closure)]


def test_every_handle_gives_back_what_it_took(ins):
    base = live(ins)
    assert base[0] >= 0 and base[1] >= 0
    for name, block in BLOCKS:
        held = block(ins)
        print("%-16s held %d buffers; after it %s, baseline %s" % (name, held, live(ins), base))
        assert held > base[0], name  # the block did allocate through the seam
        assert live(ins) == base, name
    assert live(ins) == base
