"""GPU: `ins_amd.neuralclosure` — the filtered-DNS processor inside `solve_unsteady` against the same chain on the host (filter from
tests/filter_ref.py; momentum, apply_bc_u, project from the oracle), training arrays, closure wrappers, losses and the training loop."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import filter_ref as fr
from tests.test_gpu_adjoint import _taylor
from tests.test_gpu_parity import POISSON_TOL, STEP_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def rell2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b**2)))


def axis(n):
    return np.linspace(0.0, 1.0, n + 1)


# ------------------------------------------------------------------------------------ 6. filtersaver inside solve_unsteady
def test_filtersaver_matches_host_chain(ins, oracle):
    o = oracle
    ndns, nles, savefreq, dt, nstep = 64, (16, 32), 4, 1e-3, 16
    dns = ins.Setup(x=(axis(ndns), axis(ndns)), Re=1000.0)
    les = [ins.Setup(x=(axis(n), axis(n)), Re=1000.0) for n in nles]
    comp = [ndns // n for n in nles]
    ps, ps_les = ins.psolver_spectral(dns), [ins.psolver_spectral(s) for s in les]
    filters = (ins.FaceAverage(), ins.VolumeAverage())
    u0 = ins.random_field(dns, 0.0, psolver=ps, seed=5)
    kw = dict(setup=dns, tlims=(0.0, nstep * dt), Δt=dt, psolver=ps)
    saver = ins.filtersaver(dns, les, filters, comp, ps, ps_les, nupdate=savefreq)
    (ua, _, _), out = ins.solve_unsteady(ustart=u0, processors=dict(f=saver), **kw)
    (ub, _, _), out2 = ins.solve_unsteady(ustart=u0, processors=dict(s=ins.fieldsaver(setup=dns, nupdate=savefreq)), **kw)
    (uc, _, _), _ = ins.solve_unsteady(ustart=u0, **kw)
    # the processor does not disturb the trajectory: bitwise the one with another processor at the same cadence, and the final state of the
    # plain run is reproduced to rounding (that run chains all 16 steps in one native call)
    assert bool((ua == ub).all())
    assert rell2(ins.to_numpy(ua), ins.to_numpy(uc)) < STEP_TOL
    data = out["f"]
    assert len(data) == len(les) * len(filters)
    states = [dict(u=ins.to_numpy(u0), t=0.0)] + list(out2["s"])
    assert len(states) == 5
    so = o.make_setup((axis(ndns), axis(ndns)), Re=1000.0)
    pso = o.psolver_spectral(so)
    F = [o.project(o.apply_bc_u(o.momentum(s["u"], None, s["t"], so), s["t"], so, dudt=True), so, pso) for s in states]
    k = 0
    for kind in ("face", "volume"):
        for i, n in enumerate(nles):
            d = data[k]
            k += 1
            assert d["u"].shape == (n + 2, n + 2, 2, 5) and d["c"].shape == d["u"].shape
            assert np.allclose(d["t"], [s["t"] for s in states], rtol=0, atol=1e-15)
            sl = o.make_setup((axis(n), axis(n)), Re=1000.0)
            psl = o.psolver_spectral(sl)
            for it, s in enumerate(states):
                if kind == "face":
                    Φ = lambda a: fr.face_average(a, sl.grid.Iu, sl.grid.N, comp[i])  # noqa: E731
                else:
                    Φ = lambda a: fr.volume_average(a, (n, n), comp[i])  # noqa: E731
                ubar = o.apply_bc_u(Φ(s["u"]), s["t"], sl)
                Fbar = o.project(o.apply_bc_u(o.momentum(ubar, None, s["t"], sl), s["t"], sl, dudt=True), sl, psl)
                c = Φ(F[it]) - Fbar
                inner = (slice(1, -1), slice(1, -1))
                eu, ec = rell2(d["u"][..., it], ubar), rell2(d["c"][..., it][inner], c[inner])
                print(f"{kind} n_les={n} state {it}: rell2 ū {eu:.3e}, c {ec:.3e}")
                assert eu < POISSON_TOL and ec < POISSON_TOL


def test_create_les_data_and_io_arrays(ins, tmp_path):
    files = [str(tmp_path / f"data_{i}.npz") for i in range(2)]
    data = ins.create_les_data(D=2, Re=1000.0, lims=(0.0, 1.0), nles=[16], ndns=64, filters=(ins.FaceAverage(), ins.VolumeAverage()), tburn=0.004,
                               tsim=0.012, savefreq=3, Δt=1e-3, rng=np.random.default_rng(0), filenames=files)
    assert len(data) == 2 and all(d["u"].shape == (18, 18, 2, 5) and len(d["t"]) == 5 for d in data)
    assert np.allclose(data[0]["t"], [0.0, 0.003, 0.006, 0.009, 0.012])
    saved = np.load(files[1])
    assert np.array_equal(saved["u"], data[1]["u"]) and np.array_equal(saved["c"], data[1]["c"])
    # ------------------------------------------------------------------------------------ 7. io arrays
    les = ins.Setup(x=(axis(16), axis(16)), Re=1000.0)
    io = ins.create_io_arrays(data, les)
    assert io["u"].shape == (16, 16, 2, 10) and io["c"].shape == (16, 16, 2, 10)
    for key in ("u", "c"):
        assert np.array_equal(io[key][..., :5], data[0][key][1:-1, 1:-1]) and np.array_equal(io[key][..., 5:], data[1][key][1:-1, 1:-1])


def test_collocate_decollocate_and_wrappedclosure(ins):
    import torch

    for D in (2, 3):
        rng = np.random.default_rng(D)
        a = rng.standard_normal((6,) * D + (D, 3))
        t = torch.as_tensor(a, device="cuda")
        col, dec = ins.collocate(t).cpu().numpy(), ins.decollocate(t).cpu().numpy()
        for al in range(D):
            assert np.array_equal(col[..., al, :], (a[..., al, :] + np.roll(a[..., al, :], 1, axis=al)) / 2)
            assert np.array_equal(dec[..., al, :], (a[..., al, :] + np.roll(a[..., al, :], -1, axis=al)) / 2)
    sp = ins.Setup(x=(axis(8), axis(8)), Re=1000.0)
    seen = {}

    def m(x, θ):
        seen["shape"] = tuple(x.shape)
        return θ * x * x

    wc = ins.wrappedclosure(m, sp)
    u = ins.from_numpy(sp, np.random.default_rng(1).standard_normal((10, 10, 2)))
    out = wc(u, 2.0)
    assert seen["shape"] == (8, 8, 2, 1) and tuple(out.shape) == (10, 10, 2)
    assert bool((out[1:-1, 1:-1] == 2.0 * u[1:-1, 1:-1] ** 2).all())
    assert bool((out[0] == out[-2]).all()) and bool((out[-1] == out[1]).all())
    assert bool((out[:, 0] == out[:, -2]).all()) and bool((out[:, -1] == out[:, 1]).all())


# ------------------------------------------------------------------------------------ 8. losses and training
def _les_case(ins, n=32, nstate=6, dt=2e-3, seed=2):
    """A short closure-free LES trajectory used as 'reference' data: padded states (N, N, 2, nstate) and times."""
    sp = ins.Setup(x=(axis(n), axis(n)), Re=500.0)
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    u = ins.random_field(sp, 0.0, psolver=ps, seed=seed)
    cache = ins.ode_method_cache(method, sp, ps)
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=ins.copyfield(u))
    us, ts = [ins.to_numpy(u)], [0.0]
    for _ in range(nstate - 1):
        st = ins.timestep_(method, st, dt, cache=cache)
        us.append(ins.to_numpy(st.u))
        ts.append(st.t)
    return sp, ps, method, np.stack(us, axis=-1), np.array(ts)


def _zero_cnn(ins, sp, seed=0):
    import torch

    m = ins.cnn(setup=sp, radii=[2, 2], channels=[8, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=seed)
    with torch.no_grad():
        m.convs[-1].weight.zero_()
    return m


def test_zero_closure_losses(ins):
    import torch

    sp, ps, method, U, t = _les_case(ins)
    m = _zero_cnn(ins, sp)
    # a-priori: m ≡ 0 gives Σ(0 − y)²/Σy² = 1 exactly
    rng = np.random.default_rng(0)
    x = rng.standard_normal((32, 32, 2, 4))
    y = rng.standard_normal((32, 32, 2, 4))
    loader = ins.create_dataloader_prior((x, y), batchsize=3, device=sp.device)
    batch, _ = loader(np.random.default_rng(1))
    assert tuple(batch[0].shape) == (32, 32, 2, 3)
    assert float(ins.create_loss_prior(m)(batch, None).detach()) == 1.0
    assert ins.create_relerr_prior(m, *batch)(None) == 1.0
    # a-posteriori: with m ≡ 0 the unrolled ad.timestep is the closure-free LES; perturb the reference so that the error is not zero
    Uref = U.copy()
    Uref[..., 1:] *= 1.01
    traj = dict(u=Uref, t=t)
    loss = ins.create_loss_post(setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure(m, sp))
    data, _ = ins.create_dataloader_post([traj], ntrajectory=1, nunroll=5, device=sp.device)(np.random.default_rng(0))
    assert tuple(data[0]["u"].shape) == (34, 34, 2, 6)
    with torch.no_grad():
        got = float(loss(data, None))
    inner = (slice(1, -1), slice(1, -1))
    want = np.mean([np.sum((U[..., it][inner] - Uref[..., it][inner]) ** 2) / np.sum(Uref[..., it][inner] ** 2) for it in range(1, 6)])
    print(f"loss_post with m = 0: {got:.15e}, native closure-free steps: {want:.15e}")
    # each of the 5 steps agrees with the native step to STEP_TOL (relative L2), so the relative errors (≈ 0.01 each) do to 5·STEP_TOL/0.01
    assert abs(got - want) <= 2 * 5 * STEP_TOL / 0.01 * want
    relerr = ins.create_relerr_post(data=traj, setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure(m, sp))
    e = relerr(None)
    want_e = np.mean([np.sqrt(np.sum((U[..., it][inner] - Uref[..., it][inner]) ** 2) / np.sum(Uref[..., it][inner] ** 2)) for it in range(1, 6)])
    assert abs(e - want_e) <= 5 * STEP_TOL / 0.01 * want_e


def test_loss_post_theta_gradient_taylor(ins):
    import torch

    sp, ps, method, U, t = _les_case(ins)
    U = U.copy()
    U[..., 1:] *= 1.01
    m = ins.cnn(setup=sp, radii=[1, 1], channels=[4, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=3)
    loss = ins.create_loss_post(setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure(m, sp))
    data, _ = ins.create_dataloader_post([dict(u=U, t=t)], ntrajectory=1, nunroll=5, device=sp.device)(np.random.default_rng(0))
    params = list(m.parameters())
    θ0 = torch.nn.utils.parameters_to_vector(params).detach().clone()
    gen = torch.Generator(device="cpu").manual_seed(1)
    dθ = torch.randn(θ0.numel(), generator=gen, dtype=torch.float64).to(θ0.device)
    g = torch.autograd.grad(loss(data, None), params)
    dJ = float((torch.nn.utils.parameters_to_vector(g) * dθ).sum())

    def J(e):
        with torch.no_grad():
            torch.nn.utils.vector_to_parameters(θ0 + e * dθ, params)
            val = float(loss(data, None))
            torch.nn.utils.vector_to_parameters(θ0, params)
            return val

    _taylor(J, dJ, 1e-2)


def test_train_reduces_prior_loss(ins):
    import torch

    data = ins.create_les_data(D=2, Re=1000.0, lims=(0.0, 1.0), nles=[32], ndns=128, filters=(ins.FaceAverage(),), tburn=0.01, tsim=0.04,
                               savefreq=2, Δt=1e-3, rng=np.random.default_rng(0))
    les = ins.Setup(x=(axis(32), axis(32)), Re=1000.0)
    io = ins.create_io_arrays(data, les)
    m = _zero_cnn(ins, les, seed=0)
    loss = ins.create_loss_prior(m)
    loader = ins.create_dataloader_prior((io["u"], io["c"]), batchsize=8, device=les.device)
    batch0, _ = loader(np.random.default_rng(7))
    assert float(loss(batch0, None).detach()) == 1.0
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    calls = []
    r = ins.train(dataloader=loader, loss=loss, trainstate=dict(opt=opt, θ=None, rng=np.random.default_rng(7)), niter=30,
                  callback=lambda cs, ts: calls.append(1) or cs, callbackstate=None)
    assert len(calls) == 30 and r["trainstate"]["opt"] is opt
    x, y = torch.as_tensor(io["u"], device=les.device), torch.as_tensor(io["c"], device=les.device)
    with torch.no_grad():
        final = float(loss((x, y), None))
    print(f"a-priori loss after 30 Adam iterations from the zero-output start: {final:.6f} (start 1)")
    assert final < 1.0


# ------------------------------------------------------------------------------------ 9. the example
def test_neural_closure_2d_example():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("NeuralClosure2D", os.path.join(ex, "NeuralClosure2D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.main(ndns=64, nles=16, tsim=0.02, niter=5, verbose=False)
    assert r["u"].shape == (16, 16, 2, r["nsample"]) and r["c"].shape == r["u"].shape and r["nsample"] == 2 * 11
    for k in ("prior_before", "prior_after", "post_noclosure", "post_cnn"):
        assert np.isfinite(r[k]) and r[k] >= 0
    assert r["prior_before"] == 1.0
