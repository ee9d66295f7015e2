"""The member-batched differentiable step on the device: the operator-level entries of the ensemble handle (csrc/ins_rk_ensemble.hip), the member momentum
pullback (csrc/ins_adjoint.hip, k_momentum_pullback_members_2d), the autograd Functions over them, `ad.timestep_ensemble`, `wrappedclosure_ensemble` and
`create_loss_post_ensemble`.

  1. per member every new entry is BITWISE what a B = 1 cache gives that field alone, under a permutation, with a zero member and with padding between members;
  2. the forwards agree with the single-field operators (OP_TOL / POISSON_TOL);
  3. transpose identities over the whole padded arrays, ghost volumes non-zero;
  4. the pullbacks agree with the single-field (generic) pullbacks and the momentum pullback with the dense transpose of the CPU oracle;
  5. `ad.timestep_ensemble` against `ad.timestep` per member: states and gradients to STEP_TOL, gradcheck of the two Functions;
  6. `create_loss_post_ensemble` against `create_loss_post`: value, θ-gradient, Taylor remainders, the refusal of mixed step sizes;
  7. a saved ensemble input is version checked.

Boxes: 16 x 32 (one-launch solve, one x tile), 64 x 64 (two x tiles, the 62-column seam), 128 x 16 (three-pass solve, three x tiles, fewer rows than one
y-chunk), those of tests/test_gpu_ensemble.py; B in {1, 3, 7}.  Tolerances are the existing tests' own."""
import numpy as np
import pytest
import torch

from tests import fixtures as fx
from tests.test_gpu_adjoint import TOL, _taylor, check_transpose, dense_transpose_apply, relmax
from tests.test_gpu_les_ensemble import BS, GRIDS, SENTINEL, _divfree, _padded, _pads, _setup
from tests.test_gpu_parity import OP_TOL, POISSON_TOL, STEP_TOL

pytestmark = pytest.mark.gpu

PERM = [3, 0, 6, 1, 5, 2, 4]


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def rell2(a, b):
    return float((a - b).norm() / b.norm())


def _rand(ins, sp, seed):
    """a random padded vector field, ghost volumes non-zero"""
    return ins.from_numpy(sp, 0.3 * fx.randn_field(sp.grid.N + (2,), seed))


def _fields(ins, sp, seed0):
    f = [_rand(ins, sp, seed0 + b) for b in range(max(BS))]
    f[2].zero_()  # a zero member
    return f


def _load(sp, B, fields, perm=None):
    U, flat, m = _padded(sp, B)
    for b in range(B):
        U[b].copy_(fields[perm[b] if perm else b])
    return U, flat, m


def _entries(ins):
    """name -> (run(cache, arrays) -> output array, number of input arrays, which inputs are read only)"""
    return {
        "momentum": (lambda c, F, U: ins.ensemble_momentum_(c, F, U), 2, (1,)),
        "project": (lambda c, U: ins.ensemble_project_(c, U), 1, ()),
        "apply_bc_u_pullback": (lambda c, G: ins.ensemble_apply_bc_u_pullback_(c, G), 1, ()),
        "momentum_pullback": (lambda c, Ub, P, U: ins.ensemble_momentum_pullback_(c, Ub, P, U), 3, (1, 2)),
        "momentum_pullback_acc": (lambda c, Ub, P, U: ins.ensemble_momentum_pullback_(c, Ub, P, U, accumulate=True), 3, (1, 2)),
        "project_pullback": (lambda c, G: ins.ensemble_project_pullback_(c, G), 1, ()),
    }


# ------------------------------------------------------------------------------------------------ 1. member invariance
@pytest.mark.parametrize("n", GRIDS)
def test_member_invariance(ins, n):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    rk44 = ins.RKMethods.RK44()
    sets = [_fields(ins, sp, 100), _fields(ins, sp, 200), _fields(ins, sp, 300)]  # per input slot
    live = ins.ode_method_cache(rk44, sp, ps)

    def alone():
        u = ins.apply_bc_u_(ins.copyfield(sets[0][0]), 0.0, sp)
        ins.timesteps_(rk44, ins.create_stepper(rk44, setup=sp, psolver=ps, u=u), 2e-3, 2, cache=live)
        return u

    before = alone()
    one = ins.EnsembleCache(rk44, sp, ps, 1)
    for name, (run, nin, readonly) in _entries(ins).items():
        want = []
        for b in range(max(BS)):  # B = 1 on every field alone, in the padded layout (so untouched ghost rings hold the sentinel there too)
            arrs = [_load(sp, 1, [sets[q][b]])[0] for q in range(nin)]
            want.append(run(one, *arrs)[0].clone())
        assert not torch.equal(want[0], want[1]) and float(want[0][1:-1, 1:-1].abs().max()) > 0, name
        if name != "momentum_pullback_acc":  # zero in, zero out (on the interior: the momentum's ghost ring is not written)
            assert float(want[2][1:-1, 1:-1].abs().max()) == 0.0, name
        for B in BS:
            cache = ins.EnsembleCache(rk44, sp, ps, B)
            for perm in ((None, PERM) if B == 7 else (None,)):
                loaded = [_load(sp, B, sets[q], perm) for q in range(nin)]
                keep = [flat.clone() for _, flat, _ in loaded]
                out = run(cache, *[U for U, _, _ in loaded])
                assert out is loaded[0][0]
                for q in range(nin):
                    _, flat, m = loaded[q]
                    assert bool((_pads(flat, B, m) == SENTINEL).all()), (name, B, q)  # the padding between members is untouched
                    if q in readonly:
                        assert torch.equal(flat, keep[q]), (name, B, q)  # read-only inputs are unchanged bitwise
                for b in range(B):
                    w = want[perm[b] if perm else b]
                    assert torch.equal(out[b], w), (name, n, B, b, float((out[b] - w).abs().max()))
    with pytest.raises(ValueError):
        U = ins.vectorfields(sp, 3)
        ins.ensemble_momentum_(ins.EnsembleCache(rk44, sp, ps, 3), U, U)
    # the library's own guard, behind the wrappers' host-side one: member ranges that overlap without equal base pointers are refused before any launch
    lib, c3, W = ins._lib.load(), ins.EnsembleCache(rk44, sp, ps, 3), ins.vectorfields(sp, 4)
    W.fill_(1.0)
    st = int(W.stride(0))
    assert lib.ins_rk_ensemble_momentum_f64(c3.handle, 1.0 / sp.Re, W[:3].data_ptr(), st, W[1:].data_ptr(), st, sp.stream) != 0
    assert "overlaps" in lib.ins_last_error().decode()
    assert lib.ins_rk_ensemble_momentum_pullback_f64(c3.handle, 1.0 / sp.Re, W[:3].data_ptr(), st, W[:3].data_ptr(), st, W[1:].data_ptr(), st, 0, sp.stream) != 0
    assert "overlaps" in lib.ins_last_error().decode() and bool((W == 1.0).all())
    assert torch.equal(alone(), before)  # the solver's single-field state and the live cache are as they were


# ------------------------------------------------------------------------------------------------ 2. forward parity
@pytest.mark.parametrize("n", GRIDS)
def test_forward_parity(ins, n):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    B = 3
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)
    us = [_rand(ins, sp, 10 + b) for b in range(B)]
    U = ins.vectorfields(sp, B)
    for b in range(B):
        U[b].copy_(us[b])
    F = ins.ensemble_momentum_(cache, ins.vectorfields(sp, B), U)
    P = ins.ensemble_project_(cache, U.clone())
    for b in range(B):
        ref = ins.momentum_(ins.vectorfield(sp), us[b], None, 0.0, sp)
        e = float((F[b] - ref).abs().max() / ref.abs().max())
        print(f"momentum {n} member {b}: relmax vs momentum_ {e:.3e}")
        assert e < OP_TOL
        ref = ins.apply_bc_u_(ins.project_(ins.apply_bc_u_(ins.copyfield(us[b]), 0.0, sp), sp, ps, ins.scalarfield(sp)), 0.0, sp)
        e = rell2(P[b], ref)
        print(f"project {n} member {b}: rell2 vs the per-member chain {e:.3e}")
        assert e < POISSON_TOL


# ------------------------------------------------------------------------------------------------ 3. transpose identities
@pytest.mark.parametrize("n", GRIDS)
def test_transpose_identities(ins, n):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    B = 3
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)

    def ens(seed):
        U = ins.vectorfields(sp, B)
        for b in range(B):
            U[b].copy_(_rand(ins, sp, seed + b))
        return U

    x, y, u = ens(400), ens(410), ens(420)

    def both(Lx, LTy, tol, scale_by_inputs=False):
        for a, b_, c, d in [(Lx[b], x[b], y[b], LTy[b]) for b in range(B)] + [(Lx, x, y, LTy)]:  # per member and summed
            if scale_by_inputs:
                lhs, rhs = float((a * c).sum()), float((b_ * d).sum())
                assert abs(lhs - rhs) <= tol * float(b_.norm()) * float(c.norm()), (lhs, rhs)
            else:
                check_transpose(a, b_, c, d, tol)

    both(ins.ensemble_apply_bc_u_(cache, x.clone()), ins.ensemble_apply_bc_u_pullback_(cache, y.clone()), TOL)
    both(ins.ensemble_project_(cache, x.clone()), ins.ensemble_project_pullback_(cache, y.clone()), POISSON_TOL, scale_by_inputs=True)
    # momentum is quadratic: the central difference is J(u)·x exactly (step and bound of test_convection_and_momentum_pullbacks)
    Jx = (ins.ensemble_momentum_(cache, ins.vectorfields(sp, B), u + x) - ins.ensemble_momentum_(cache, ins.vectorfields(sp, B), u - x)) / 2
    both(Jx, ins.ensemble_momentum_pullback_(cache, ins.vectorfields(sp, B), y, u), TOL)


# ------------------------------------------------------------------------------------------------ 4. pullback parity
@pytest.mark.parametrize("n", GRIDS)
def test_pullback_parity(ins, n):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    B = 3
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)
    us, ws, bases = ([_rand(ins, sp, s + b) for b in range(B)] for s in (500, 510, 520))
    U, W, Base = ins.vectorfields(sp, B), ins.vectorfields(sp, B), ins.vectorfields(sp, B)
    for b in range(B):
        U[b].copy_(us[b])
        W[b].copy_(ws[b])
        Base[b].copy_(bases[b])
    got = ins.ensemble_momentum_pullback_(cache, ins.vectorfields(sp, B), W, U)
    acc = ins.ensemble_momentum_pullback_(cache, Base.clone(), W, U, accumulate=True)
    pp = ins.ensemble_project_pullback_(cache, W.clone())
    for b in range(B):
        ref = ins.momentum_pullback_(ins.vectorfield(sp), ws[b], us[b], sp)  # the generic kernel: the bound of test_tiled_momentum_pullback_matches_generic
        assert float((got[b] - ref).abs().max()) <= TOL * float(ref.abs().max()), (n, b)
        refa = ins.momentum_pullback_(ins.copyfield(bases[b]), ws[b], us[b], sp, accumulate=True)
        assert float((acc[b] - refa).abs().max()) <= TOL * float(refa.abs().max()), (n, b)
        g = ins.apply_bc_u_pullback_(ins.copyfield(ws[b]), 0.0, sp)
        ins.project_pullback_(g, sp, ps, ins.scalarfield(sp))
        ins.apply_bc_u_pullback_(g, 0.0, sp)
        e = rell2(pp[b], g)
        print(f"project pullback {n} member {b}: rell2 vs the per-member chain {e:.3e}")
        assert e < POISSON_TOL


def test_momentum_pullback_matches_oracle_transpose(ins, oracle):
    """value by value against the dense transpose of the CPU oracle's momentum (unit probes), as test_pullbacks_match_oracle_transposes"""
    o = oracle
    x = tuple(np.linspace(0.0, 1.0, ni + 1) for ni in (16, 32))
    so = o.make_setup(x, Re=500.0)
    sp = _setup(ins, (16, 32))
    ps = ins.psolver_spectral(sp)
    B = 3
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)
    vs = tuple(so.grid.N) + (2,)
    u, w = 0.3 * fx.randn_field(vs, 20), fx.randn_field(vs, 21)
    U, W = ins.vectorfields(sp, B), ins.vectorfields(sp, B)
    U[1].copy_(ins.from_numpy(sp, u))
    W[1].copy_(ins.from_numpy(sp, w))
    got = ins.ensemble_momentum_pullback_(cache, ins.vectorfields(sp, B), W, U)
    ref = dense_transpose_apply(lambda e: (o.momentum(u + e, None, 0.0, so) - o.momentum(u - e, None, 0.0, so)) / 2, vs, w)
    err = relmax(ins.to_numpy(got[1]), ref)
    assert err <= TOL, err
    assert not bool(got[0].any()) and not bool(got[2].any())


# ------------------------------------------------------------------------------------------------ 5. the step
def _small_cnn(ins, sp, batched=False):
    return ins.cnn(setup=sp, radii=[1, 1], channels=[4, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=3, batched=batched)


@pytest.mark.parametrize("n", GRIDS)
def test_batched_cnn_matches_the_cnn_on_the_device(ins, n):
    """`cnn(..., batched=True)` (all members one sample in the convolutions) against the plain network with the same weights, through
    `wrappedclosure_ensemble`: values and parameter gradients to 1e-13 relative to the largest value (a dot product of at most 4·9 terms summed in another
    order, two layers, then the gradient's sums: a few hundred eps)."""
    sp = _setup(ins, n)
    B = 7
    U = ins.vectorfields(sp, B)
    for b in range(B):
        U[b].copy_(_rand(ins, sp, 700 + b))
    res = []
    for batched in (False, True):
        m = _small_cnn(ins, sp, batched)
        y = ins.wrappedclosure_ensemble(m, sp)(U, None)
        assert tuple(y.shape) == tuple(U.shape) and tuple(y.stride()) == tuple(U.stride())
        res.append((y.detach(), torch.autograd.grad((y * y).sum(), list(m.parameters()))))
    (ya, ga), (yb, gb) = res
    assert float(ya.abs().max()) > 0 and float((ya - yb).abs().max()) <= 1e-13 * float(ya.abs().max())
    for p, q in zip(ga, gb):
        assert float((p - q).abs().max()) <= 1e-13 * float(p.abs().max())


def _ke(u):
    v = u[..., 1:-1, 1:-1, :]
    return (v * v).sum()


@pytest.mark.parametrize("method", ["RK44", "Wray3"])
@pytest.mark.parametrize("n", GRIDS)
def test_timestep_ensemble_matches_per_member(ins, n, method):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    rk = getattr(ins.RKMethods, method)()
    dt = 1e-3
    m = _small_cnn(ins, sp)
    params = list(m.parameters())
    starts = [_divfree(ins, sp, ps, 30 + b) for b in range(max(BS))]
    worst = {}
    for closed in (False, True):
        spm = ins.neuralclosure._SetupView(sp, ins.wrappedclosure(m, sp)) if closed else sp
        # per member: once, shared by every B
        ref = []
        for u0 in starts:
            uu = u0.clone().requires_grad_(True)
            st = ins.create_stepper(rk, setup=spm, psolver=ps, u=uu)
            states = []
            for _ in range(3):
                st = ins.ad.timestep(rk, st, dt, None)
                states.append(st.u)
            g = torch.autograd.grad(_ke(states[-1]), [uu] + (params if closed else []))
            ref.append((states[0].detach(), states[2].detach(), g[0], torch.nn.utils.parameters_to_vector(g[1:]) if closed else None))
        for B in BS:
            cache = ins.EnsembleCache(rk, sp, ps, B)
            U0 = ins.vectorfields(sp, B)
            for b in range(B):
                U0[b].copy_(starts[b])
            U0.requires_grad_(True)
            closure = ins.wrappedclosure_ensemble(m, sp) if closed else None
            U, states = U0, []
            for _ in range(3):
                U = ins.ad.timestep_ensemble(rk, cache, U, 0.0, dt, None, closure)
                states.append(U)
            g = torch.autograd.grad(_ke(states[-1]), [U0] + (params if closed else []))
            errs = [max(rell2(states[0][b].detach(), ref[b][0]) for b in range(B)), max(rell2(states[2][b].detach(), ref[b][1]) for b in range(B)),
                    max(rell2(g[0][b], ref[b][2]) for b in range(B))]
            if closed:
                errs.append(rell2(torch.nn.utils.parameters_to_vector(g[1:]), sum(ref[b][3] for b in range(B))))
            print(f"timestep_ensemble {n} {method} closure={closed} B={B}: rell2 state 1 step {errs[0]:.3e}, 3 steps {errs[1]:.3e}, dL/dU0 {errs[2]:.3e}"
                  + (f", dL/dθ {errs[3]:.3e}" if closed else ""))
            assert all(e < STEP_TOL for e in errs), (n, method, closed, B, errs)
            worst[closed] = max(worst.get(closed, 0.0), *errs)
    print(f"timestep_ensemble {n} {method}: worst rell2 without closure {worst[False]:.3e}, with the CNN {worst[True]:.3e}")


@pytest.mark.parametrize("which", ["momentum", "project"])
def test_gradcheck_member_functions(ins, which):
    """the settings of test_gradcheck_right_hand_side, on 16 x 32 with B = 2"""
    sp = _setup(ins, (16, 32))
    ps = ins.psolver_spectral(sp)
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, 2)
    U = ins.vectorfields(sp, 2)
    for b in range(2):
        U[b].copy_(_rand(ins, sp, 30 + b))
    U.requires_grad_(True)
    f = ins.ad.ensemble_momentum if which == "momentum" else ins.ad.ensemble_project
    assert torch.autograd.gradcheck(lambda uu: f(cache, uu), (U,), eps=1e-6, atol=1e-6, rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 6. the loss
def _batch(ins, sp, ps, method, ntraj=3, nstate=4, dt=2e-3):
    """`ntraj` short closure-free LES trajectories with their own start times, the later states scaled so that the error is not zero"""
    cache = ins.ode_method_cache(method, sp, ps)
    data = []
    for k in range(ntraj):
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=ins.random_field(sp, 0.0, psolver=ps, seed=60 + k), t=0.1 * k)
        us, ts = [st.u.clone()], [st.t]
        for _ in range(nstate - 1):
            st = ins.timestep_(method, st, dt, cache=cache)
            us.append(1.01 * st.u)
            ts.append(st.t)
        data.append(dict(u=torch.stack(us, dim=-1), t=np.array(ts)))
    return data


def test_loss_post_ensemble_matches_loss_post(ins):
    sp = _setup(ins, (32, 32))
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    m, mb = _small_cnn(ins, sp), _small_cnn(ins, sp, batched=True)  # same seed, same weights: the loop's network and the ensemble's batched one
    params = list(mb.parameters())
    data = _batch(ins, sp, ps, method)
    loop = ins.create_loss_post(setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure(m, sp))
    ens = ins.create_loss_post_ensemble(setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure_ensemble(mb, sp))
    Lr = loop(data, None)
    gr = torch.nn.utils.parameters_to_vector(torch.autograd.grad(Lr, list(m.parameters())))
    Le = ens(data, None)
    ge = torch.nn.utils.parameters_to_vector(torch.autograd.grad(Le, params))
    Le, Lr = Le.detach(), Lr.detach()
    ev, eg = abs(float(Le) - float(Lr)) / abs(float(Lr)), rell2(ge, gr)
    print(f"loss_post_ensemble vs loss_post: value {float(Le):.15e} / {float(Lr):.15e} (rel {ev:.3e}), θ-gradient rell2 {eg:.3e}")
    assert ev < STEP_TOL and eg < STEP_TOL
    # Taylor remainders in θ (test_loss_post_theta_gradient_taylor)
    θ0 = torch.nn.utils.parameters_to_vector(params).detach().clone()
    dθ = torch.randn(θ0.numel(), generator=torch.Generator(device="cpu").manual_seed(1), dtype=torch.float64).to(θ0.device)
    dJ = float((ge * dθ).sum())

    def J(e):
        with torch.no_grad():
            torch.nn.utils.vector_to_parameters(θ0 + e * dθ, params)
            val = float(ens(data, None))
            torch.nn.utils.vector_to_parameters(θ0, params)
            return val

    _taylor(J, dJ, 1e-2)
    # a batch with unequal step sizes, and one with unequal lengths
    bad = [dict(u=d["u"], t=d["t"].copy()) for d in data]
    bad[1]["t"][2:] += 1e-3
    with pytest.raises(ValueError) as e:
        ens(bad, None)
    assert "create_loss_post" in str(e.value)
    with pytest.raises(ValueError) as e:
        ens([data[0], dict(u=data[1]["u"][..., :3], t=data[1]["t"][:3])], None)
    assert "create_loss_post" in str(e.value)


# ------------------------------------------------------------------------------------------------ 7. version check
def test_saved_ensemble_input_is_version_checked(ins):
    sp = _setup(ins, (16, 32))
    ps = ins.psolver_spectral(sp)
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, 2)
    U = ins.vectorfields(sp, 2)
    for b in range(2):
        U[b].copy_(_rand(ins, sp, 64 + b))
    U.requires_grad_(True)
    out = ins.ad.ensemble_momentum(cache, U)
    with torch.no_grad():
        U.add_(1.0)
    with pytest.raises(RuntimeError):
        out.backward(torch.ones_like(out))
