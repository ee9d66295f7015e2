"""The routes of live Float32 handles (csrc/ins_f32.hip): a created solver's route is the one ins_f32_choose gives for its box, and the step's route record
(rk32_route, read through ins_dbg_rk32_route) is what the conditions of the stage loops were before they were one function: which boxes take the wide
stage kernel, the in-register correction, the stage-velocity basis and chained steps, and which switches clear which of them on a handle that exists.
Handles are only created, and one case steps three times."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HIPFFT, FP64_SPECTRA, FLOAT2_SPECTRA, WRAP = range(4)  # F32Route of csrc/ins_f32_internal.h
GENERAL, WIDE, INCORR, FLOAT2, VBASIS, CHAINABLE = 1, 2, 4, 8, 16, 32  # the bit set of ins_dbg_rk32_route (csrc/ins_debug.h)

BOXES = [(32, 32), (66, 12, 10), (24, 18), (128, 16, 16), (32, 16, 16), (128, 16, 256), (256, 16, 192)]


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def exact(n):
    """uniform spacings that are exact binary fractions (the in-register correction needs them)"""
    return tuple(np.arange(ni + 1) / 2.0 ** int(np.ceil(np.log2(ni))) for ni in n)


def walls24(ins):
    Dn, P = ins.DirichletBC, ins.PeriodicBC
    x = (np.tanh(1.2 * (2 * np.linspace(0.0, 1.0, 25) - 1)) / np.tanh(1.2) / 2 + 0.5, (1 - np.cos(np.pi * np.arange(11) / 10)) / 2, np.linspace(-0.2, 0.2, 9))
    return ins.Setup(x=x, Re=500.0, boundary_conditions=((Dn(), Dn()), (Dn(), Dn((1.0, 0.2, 0.0))), (P(), P())))


def route_of(ins, cache):
    flags = C.c_int32(-1)
    route = ins._lib.load().ins_dbg_rk32_route(cache._handle, C.byref(flags))
    return route, flags.value


def chosen(ins, n):
    return ins._lib.load().ins_dbg_f32_choose(len(n), *(tuple(n) + (1,) * (3 - len(n))))


@pytest.mark.parametrize("n", BOXES)
def test_created_solver_is_on_the_chosen_route(ins, n):
    f32 = ins.f32
    sp = ins.Setup(x=exact(n), Re=500.0)
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    route, flags = route_of(ins, cache)
    assert route == chosen(ins, n)
    assert route == {(128, 16, 16): FP64_SPECTRA, (32, 16, 16): FP64_SPECTRA, (128, 16, 256): FLOAT2_SPECTRA, (256, 16, 192): FLOAT2_SPECTRA}.get(n, HIPFFT)
    assert not flags & GENERAL
    assert bool(flags & FLOAT2) == (route == FLOAT2_SPECTRA)
    if route == HIPFFT:  # no pressure of own passes to correct with in registers
        assert not flags & (INCORR | VBASIS | CHAINABLE)
    del cache, ps


@pytest.mark.parametrize("n,method,want", [((128, 16, 256), "RK44", WIDE | INCORR | FLOAT2 | VBASIS | CHAINABLE),
                                           ((128, 16, 16), "RK44", WIDE | INCORR | VBASIS),
                                           ((32, 16, 16), "RK44", 0),
                                           ((128, 16, 256), "FE11", WIDE | FLOAT2)])  # one stage: nothing to correct in registers
def test_step_route_of_a_periodic_box(ins, n, method, want):
    f32 = ins.f32
    sp = ins.Setup(x=exact(n), Re=500.0)
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(getattr(ins.RKMethods, method)(), sp, ps)
    assert route_of(ins, cache)[1] == want
    del cache, ps


def test_step_route_of_a_wrapped_solver(ins):
    f32 = ins.f32
    sp = walls24(ins)
    ps = f32.default_psolver32(sp)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    assert route_of(ins, cache) == (WRAP, GENERAL)
    del cache, ps
    # a wrapped solver on a periodic uniform box: the wrapped route without `general`, the row of ADVICE.md's first finding (the step takes the periodic
    # loop without the ghost fills the wrapped projection needs); pinned as the route it is, not as a behaviour to keep
    sp = ins.Setup(x=exact((32, 16, 16)), Re=500.0)
    ps = f32.psolver_wrap32(sp, ins.psolver_spectral(sp))
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    assert route_of(ins, cache) == (WRAP, 0)
    del cache, ps


def test_switches_clear_their_flags_on_a_live_handle(ins):
    f32 = ins.f32
    sp = ins.Setup(x=exact((128, 16, 256)), Re=500.0)
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    full = WIDE | INCORR | FLOAT2 | VBASIS | CHAINABLE
    assert route_of(ins, cache) == (FLOAT2_SPECTRA, full)
    for opt, cleared in (("INS_DISABLE_INKERNEL_CORR", INCORR | VBASIS | CHAINABLE), ("INS_RK_KEEP_K", VBASIS | CHAINABLE),
                         ("INS_DISABLE_STEP_CHAIN", CHAINABLE)):
        with ins._lib.options(**{opt: 1}):
            assert route_of(ins, cache) == (FLOAT2_SPECTRA, full & ~cleared), opt
        assert route_of(ins, cache) == (FLOAT2_SPECTRA, full)
    # the solver's route is frozen at creation: the switches that choose it do not move a handle that exists
    with ins._lib.options(INS_F32_FP64_SPECTRA=1, INS_F32_HIPFFT_PROJECT=1, INS_F32_SPLIT_GRADIENT=1):
        assert route_of(ins, cache) == (FLOAT2_SPECTRA, full)
        assert chosen(ins, (128, 16, 256)) == HIPFFT
    del cache, ps


def test_steps_on_a_handle_that_does_not_chain_are_single_steps(ins):
    f32 = ins.f32
    n = (128, 16, 16)
    sp = ins.Setup(x=exact(n), Re=500.0)
    ps = f32.psolver_spectral32(sp)
    cache = f32.ERKCache32(ins.RKMethods.RK44(), sp, ps)
    assert not route_of(ins, cache)[1] & CHAINABLE
    u0 = f32.to_f32(sp, np.asfortranarray(0.1 * np.random.default_rng(5).standard_normal(sp.grid.N + (3,))))
    f32.project32_(u0, sp, ps, f32.scalarfield32(sp))
    a, b = u0.clone(), u0.clone()
    f32.timesteps32_(cache, a, 1e-3, 3)
    for _ in range(3):
        f32.timestep32_(cache, b, 1e-3)
    assert torch.isfinite(a).all() and not torch.equal(a, u0)
    assert torch.equal(a, b)
    del cache, ps
