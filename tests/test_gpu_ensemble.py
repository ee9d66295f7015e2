"""Ensemble stepping (`vectorfields`, `EnsembleCache`, `timesteps_ensemble_`; csrc/ins_rk_ensemble.hip): B independent 2-D periodic flows advanced by one
native loop whose launches each carry all members.  Every comparison here is `torch.equal`: member b after `nsteps` is BITWISE what `timesteps_` gives that
field alone with a fresh `ERKCache`, for every branch of the loop —
  16 x 32   the one-launch solve (k_xysolve2d), anisotropic, one x tile of the stage kernel,
  64 x 64   the one-launch solve, two 62-column tiles,
  128 x 16  the three-pass solve (x forward, fused y solve, x inverse), three x tiles, anisotropic;
  nsteps 1 / 2 / 5: the unchained step, first + last step of a chain, a chain's middle steps;  B = 1, 3, 7;
  RK44, SSP33 and LMWray3 (as the explicit method it is): between them zero and non-zero coefficients below the diagonal of A."""
import numpy as np
import pytest
import torch

from tests import fixtures as fx

pytestmark = pytest.mark.gpu

GRIDS = [(16, 32), (64, 64), (128, 16)]
BS = (1, 3, 7)
NSTEPS = (1, 2, 5)
DT = 2e-3


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def _method(ins, name):
    return ins.LMWray3() if name == "LMWray3" else getattr(ins.RKMethods, name)()


def _problem(ins, n, Re=500.0):
    x = tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n)
    sp = ins.Setup(x=x, Re=Re, device="cuda:0")
    return sp, ins.psolver_spectral(sp)


def _divfree(ins, sp, ps, seed):
    """A random field made divergence-free by the projection, ghost volumes filled: what every member starts from (different per seed)."""
    u = ins.from_numpy(sp, 0.3 * fx.randn_field(sp.grid.N + (2,), seed))
    ins.apply_bc_u_(u, 0.0, sp)
    ins.project_(u, sp, ps, ins.scalarfield(sp))
    return ins.apply_bc_u_(u, 0.0, sp)


def _alone(ins, method, sp, ps, u0, nsteps):
    """`timesteps_` on a copy of one member with a fresh cache: the reference of every comparison."""
    u = ins.copyfield(u0)
    cache = ins.ode_method_cache(method, sp, ps)
    ins.timesteps_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u), DT, nsteps, cache=cache)
    return u


def _ensemble(ins, sp, members):
    U = ins.vectorfields(sp, len(members))
    for b, u in enumerate(members):
        U[b].copy_(u)
    return U


@pytest.mark.parametrize("name", ["RK44", "SSP33", "LMWray3"])
@pytest.mark.parametrize("n", GRIDS)
def test_every_member_is_bitwise_timesteps_alone(ins, n, name):
    sp, ps = _problem(ins, n)
    method = _method(ins, name)
    if name != "LMWray3":
        A = np.tril(method.A, -1)
        assert (name == "RK44") == bool((A[np.tril_indices_from(A, -1)] == 0).any())  # RK44 has zeros below the diagonal, SSP33 none
    starts = [_divfree(ins, sp, ps, 10 + b) for b in range(max(BS))]
    assert not torch.equal(starts[0], starts[1])
    want = {ns: [_alone(ins, method, sp, ps, u0, ns) for u0 in starts] for ns in NSTEPS}  # once, shared by every B
    assert not torch.equal(want[1][0], starts[0]) and not torch.equal(want[5][0], want[2][0])
    for B in BS:
        cache = ins.EnsembleCache(method, sp, ps, B)
        for ns in NSTEPS:
            U = _ensemble(ins, sp, starts[:B])
            assert tuple(U.shape) == (B,) + sp.grid.N + (2,) and U[B - 1].stride() == ins.vectorfield(sp).stride()
            out = ins.timesteps_ensemble_(cache, U, 0.0, DT, ns)
            assert out is U
            for b in range(B):
                assert torch.equal(U[b], want[ns][b]), (n, name, B, ns, b, float((U[b] - want[ns][b]).abs().max()))
    # every existing operator takes a member unchanged: ghosts valid, divergence-free
    assert ins.max_abs_divergence(U[B - 1], sp) < 1e-10 and torch.equal(ins.apply_bc_u(U[0], 0.0, sp), U[0])


@pytest.mark.parametrize("n", [(64, 64), (128, 16)])  # one box per solve route
def test_members_do_not_see_each_other(ins, n):
    sp, ps = _problem(ins, n)
    method = ins.RKMethods.RK44()
    starts = [_divfree(ins, sp, ps, 20 + b) for b in range(3)]
    cache = ins.EnsembleCache(method, sp, ps, 3)
    base = ins.timesteps_ensemble_(cache, _ensemble(ins, sp, starts), 0.0, DT, 3)
    # permuting the members permutes the results
    perm = [2, 0, 1]
    got = ins.timesteps_ensemble_(cache, _ensemble(ins, sp, [starts[q] for q in perm]), 0.0, DT, 3)
    for b, q in enumerate(perm):
        assert torch.equal(got[b], base[q])
    # member 1 replaced by zeros: it stays zero, members 0 and 2 do not change by a bit
    got = ins.timesteps_ensemble_(cache, _ensemble(ins, sp, [starts[0], torch.zeros_like(starts[1]), starts[2]]), 0.0, DT, 3)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and not got[1].any()


@pytest.mark.parametrize("n", [(16, 32), (128, 16)])
def test_padding_between_members_is_untouched(ins, n):
    sp, ps = _problem(ins, n)
    method = ins.RKMethods.RK44()
    B, pad, sentinel = 3, 37, -7.25
    nvec = int(np.prod(sp.grid.N)) * 2
    stride = nvec + pad
    buf = torch.full((pad + B * stride,), sentinel, dtype=torch.float64, device=sp.device)
    N0, N1 = sp.grid.N
    U = buf[pad:].as_strided((B, N0, N1, 2), (stride, 1, N0, N0 * N1))
    starts = [_divfree(ins, sp, ps, 30 + b) for b in range(B)]
    for b in range(B):
        U[b].copy_(starts[b])
    ins.timesteps_ensemble_(ins.EnsembleCache(method, sp, ps, B), U, 0.0, DT, 2)
    for b in range(B):
        assert torch.equal(U[b], _alone(ins, method, sp, ps, starts[b], 2))
        assert bool((buf[pad + b * stride + nvec: pad + (b + 1) * stride] == sentinel).all())
    assert bool((buf[:pad] == sentinel).all())


@pytest.mark.parametrize("n", [(32, 32), (128, 16)])
def test_solver_and_single_field_cache_are_not_disturbed(ins, n):
    """The psolver and an ERKCache of the same setup, used before and after an ensemble call, give what they give without it."""
    sp, ps = _problem(ins, n)
    method = ins.RKMethods.RK44()
    starts = [_divfree(ins, sp, ps, 40 + b) for b in range(3)]
    f = ins.from_numpy(sp, fx.randn_field(sp.grid.N, 3))
    want_p = ps(ins.copyfield(f))
    want_u = _alone(ins, method, sp, ps, _alone(ins, method, sp, ps, starts[0], 2), 2)  # two calls of two steps, nothing in between
    # the same two halves with an ensemble call in between, on ONE single-field cache
    cache = ins.ode_method_cache(method, sp, ps)
    u = ins.copyfield(starts[0])
    st = ins.timesteps_(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u), DT, 2, cache=cache)
    ens = ins.EnsembleCache(method, sp, ps, 3)
    ins.timesteps_ensemble_(ens, _ensemble(ins, sp, starts), 0.0, DT, 3)
    assert torch.equal(ps(ins.copyfield(f)), want_p)
    ins.timesteps_(method, st, DT, 2, cache=cache)
    assert torch.equal(u, want_u)


def test_refusals_name_the_per_member_route(ins):
    """Outside the chained 2-D loop nothing is launched: NotImplementedError naming `timesteps_` per member."""
    rk44 = ins.RKMethods.RK44()
    per, dbc = (ins.PeriodicBC(), ins.PeriodicBC()), (ins.DirichletBC(), ins.DirichletBC())
    x2 = tuple(np.linspace(0.0, 1.0, 33) for _ in range(2))

    def refused(method, sp, ps, what):
        with pytest.raises(NotImplementedError, match=what) as e:
            ins.EnsembleCache(method, sp, ps, 4)
        assert "timesteps_" in str(e.value) and "per member" in str(e.value)

    sp = ins.Setup(x=tuple(np.linspace(0.0, 1.0, 17) for _ in range(3)), Re=500.0, device="cuda:0")
    refused(rk44, sp, ins.psolver_spectral(sp), "3-D")
    sp = ins.Setup(x=x2, boundary_conditions=(per, dbc), Re=500.0, device="cuda:0")
    refused(rk44, sp, ins.psolver_direct(sp), "not periodic")
    sp = ins.Setup(x=(np.linspace(0.0, 1.0, 49), np.linspace(0.0, 1.0, 33)), Re=500.0, device="cuda:0")  # a side of 48: the rocFFT route
    refused(rk44, sp, ins.psolver_spectral(sp), "48 x 32")
    sp = ins.Setup(x=x2, Re=500.0, bodyforce=lambda a, x, y, t: (a == 0) * np.sin(2 * np.pi * y) + 0 * x, issteadybodyforce=True, device="cuda:0")
    refused(rk44, sp, ins.psolver_spectral(sp), "body force")
    sp = ins.Setup(x=x2, Re=500.0, closure_model=lambda u, θ: 0 * u, device="cuda:0")
    refused(rk44, sp, ins.psolver_spectral(sp), "closure")
    T = ins.temperature_equation(Pr=0.71, Ra=1e5, Ge=0.1, boundary_conditions=(per, per))
    sp = ins.Setup(x=x2, temperature=T, device="cuda:0")
    refused(rk44, sp, ins.psolver_spectral(sp), "temperature")
    sp = ins.Setup(x=x2, Re=500.0, device="cuda:0")
    ps = ins.psolver_spectral(sp)
    refused(ins.RKMethods.FE11(), sp, ps, "one-stage")
    # and the library's own entry refuses what its predicate turns away (here: a one-stage tableau handed to it directly)
    import ctypes as C

    lib, h = ins._lib.load(), C.c_void_p()
    one = np.ones(1)
    dp = ins._lib.c_double_p
    assert lib.ins_rk_ensemble_create(sp.handle, ps.handle, 1, one.ctypes.data_as(dp), one.ctypes.data_as(dp), 4, C.byref(h)) == -4 and not h.value
    assert b"ins_rk_steps_f64" in lib.ins_last_error() and b"per member" in lib.ins_last_error()
    # a cache for B members takes B members
    with pytest.raises(ValueError, match="B = 4"):
        ins.timesteps_ensemble_(ins.EnsembleCache(rk44, sp, ps, 4), ins.vectorfields(sp, 3), 0.0, DT, 1)
