"""GPU: `ins_amd.neuralclosure` on a Float32 run — the filtered-DNS processor inside the Float32 `solve_unsteady` against the hand chain of the
public Float32 functions (bitwise) and against the fp64 pipeline, Float32 data generation, and the Float32 training glue."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_adjoint import mirror
from tests.test_gpu_solve32 import STEP_TOL

pytestmark = pytest.mark.gpu

# ‖c32 − c64‖ / ‖ΦF64‖ of the filtersaver test below (64² -> 16², 32², both filters, five states): the largest value measured on an MI355X is
# C_MEASURED; the assertion allows four times that for the spread between seeds (DESIGN.md §6c "Float32").
C_MEASURED = 9.025e-7  # over the 2 filters x 2 grids x 5 states; c compared on the degrees of freedom
C_TOL = 4 * C_MEASURED


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def rell2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b**2)))


def axis(n):
    return np.linspace(0.0, 1.0, n + 1)


def hand_chain32(ins, u, dns, les, Φ, comp, ps_dns, ps_les):
    """(ū, c) of one float32 DNS state from the public Float32 functions (data_generation.jl:37-60, 88-100)."""
    f32 = ins.f32
    F = f32.momentum32_(f32.vectorfield32(dns), u, dns)
    f32.project32_(f32.apply_bc_u32_(F, dns, dudt=True), dns, ps_dns, f32.scalarfield32(dns))
    Φu = f32.apply_bc_u32_(Φ(u, les, comp, setup_dns=dns), les)
    ΦF = Φ(F, les, comp, setup_dns=dns)
    FΦ = f32.momentum32_(f32.vectorfield32(les), Φu, les)
    f32.project32_(f32.apply_bc_u32_(FΦ, les, dudt=True), les, ps_les, f32.scalarfield32(les))
    return ins.to_numpy(Φu), ins.to_numpy(ΦF - FΦ)


# ------------------------------------------------------------------------------------ 1. filtersaver on a float32 run
def test_filtersaver32(ins):
    f32 = ins.f32
    ndns, nles, savefreq, dt, nstep = 64, (16, 32), 4, 1e-3, 16
    dns = ins.Setup(x=(axis(ndns), axis(ndns)), Re=1000.0)
    les = [ins.Setup(x=(axis(n), axis(n)), Re=1000.0) for n in nles]
    comp = [ndns // n for n in nles]
    ps, ps_les = f32.psolver_spectral32(dns), [f32.psolver_spectral32(s) for s in les]
    ps64, ps64_les = ins.psolver_spectral(dns), [ins.psolver_spectral(s) for s in les]
    filters = (ins.FaceAverage(), ins.VolumeAverage())
    u0 = f32.to_f32(dns, ins.random_field(dns, 0.0, psolver=ps64, seed=5))
    keep = u0.clone()
    kw = dict(setup=dns, tlims=(0.0, nstep * dt), Δt=dt)
    saver = ins.filtersaver(dns, les, filters, comp, ps, ps_les, nupdate=savefreq)
    (ua, _, _), out = ins.solve_unsteady(ustart=u0, psolver=ps, processors=dict(f=saver), **kw)
    (ub, _, _), out2 = ins.solve_unsteady(ustart=u0, psolver=ps, processors=dict(s=ins.fieldsaver(setup=dns, nupdate=savefreq)), **kw)
    # the processor does not disturb the trajectory, nor the start field
    assert bool((ua == ub).all()) and bool((u0 == keep).all())
    data = out["f"]
    states = [dict(u=ins.to_numpy(u0), t=0.0)] + list(out2["s"])
    assert len(data) == len(les) * len(filters) and len(states) == 5
    # the fp64 pipeline from the same rounded field
    saver64 = ins.filtersaver(dns, les, filters, comp, ps64, ps64_les, nupdate=savefreq)
    _, out64 = ins.solve_unsteady(ustart=u0.double(), psolver=ps64,
                                  processors=dict(f=saver64, s=ins.fieldsaver(setup=dns, nupdate=savefreq)), **kw)
    states64 = [dict(u=ins.to_numpy(u0.double()), t=0.0)] + list(out64["s"])
    F64 = []
    for s in states64:
        F = ins.momentum_(ins.vectorfield(dns), ins.from_numpy(dns, s["u"]), None, s["t"], dns)
        F64.append(ins.project_(ins.apply_bc_u_(F, s["t"], dns, dudt=True), dns, ps64, ins.scalarfield(dns)))
    k, cmax, inner = 0, 0.0, (slice(1, -1), slice(1, -1))
    for Φ in filters:
        for i, n in enumerate(nles):
            d, d64 = data[k], out64["f"][k]
            k += 1
            assert d["u"].dtype == np.float32 and d["c"].dtype == np.float32 and d["t"].dtype == np.float64
            assert d["u"].shape == (n + 2, n + 2, 2, 5) and d["c"].shape == d["u"].shape
            assert np.allclose(d["t"], [s["t"] for s in states], rtol=0, atol=1e-15)
            for it, s in enumerate(states):
                ubar, c = hand_chain32(ins, f32.to_f32(dns, s["u"]), dns, les[i], Φ, comp[i], ps, ps_les[i])
                assert np.array_equal(d["u"][..., it], ubar) and np.array_equal(d["c"][..., it], c)
                # c on the degrees of freedom (what create_io_arrays keeps): the filters write Iu only, and the ghosts of a projected field are
                # the solver's business (the fp64 spectral projection leaves them, the Float32 one refills them)
                ΦF64 = ins.to_numpy(Φ(F64[it], les[i], comp[i], setup_dns=dns))[inner]
                eu = rell2(d["u"][..., it], d64["u"][..., it])
                ec = float(np.linalg.norm(d["c"][..., it][inner].astype(np.float64) - d64["c"][..., it][inner]) / np.linalg.norm(ΦF64))
                cmax = max(cmax, ec)
                print(f"{Φ} n_les={n} state {it}: rell2 ū32 vs ū64 {eu:.3e}, |c32 - c64| / |ΦF64| {ec:.3e}")
                assert eu < STEP_TOL
                assert ec < C_TOL
    print(f"largest |c32 - c64| / |ΦF64| = {cmax:.3e}")


# ------------------------------------------------------------------------------------ 2. wall-bounded
def test_filtersaver32_wall_bounded(ins, oracle):
    f32 = ins.f32
    les = mirror(ins, fx.setup2d(oracle), oracle)
    dns = ins.neuralclosure.dns_setup_of(les, 2)
    ps, ps_les = f32.psolver_wrap32(dns), f32.psolver_wrap32(les)
    Φ = ins.FaceAverage()
    u = f32.apply_bc_u32_(f32.to_f32(dns, fx.randn_field(tuple(dns.grid.N) + (2,), 3)), dns)
    keep = u.clone()
    saver = ins.filtersaver(dns, [les], [Φ], [2], ps, [ps_les], nupdate=1)
    state = dict(u=u, temp=None, t=0.0, n=0)
    (d,) = saver.finalize(saver.initialize(lambda: state), lambda: state)
    assert bool((u == keep).all())
    assert d["u"].dtype == np.float32 and d["u"].shape == tuple(les.grid.N) + (2, 1) and list(d["t"]) == [0.0]
    ubar, c = hand_chain32(ins, u, dns, les, Φ, 2, ps, ps_les)
    assert np.array_equal(d["u"][..., 0], ubar) and np.array_equal(d["c"][..., 0], c)
    assert np.isfinite(c).all() and np.abs(c).max() > 0


# ------------------------------------------------------------------------------------ 3. create_les_data(dtype=torch.float32)
@pytest.fixture(scope="module")
def les_data32(ins, tmp_path_factory):
    import torch

    tmp = tmp_path_factory.mktemp("les32")
    files = [str(tmp / f"data_{i}.npz") for i in range(2)]
    data = ins.create_les_data(D=2, Re=1000.0, lims=(0.0, 1.0), nles=[16], ndns=64, filters=(ins.FaceAverage(), ins.VolumeAverage()), tburn=0.004,
                               tsim=0.012, savefreq=3, Δt=1e-3, rng=np.random.default_rng(0), filenames=files, dtype=torch.float32)
    return data, files


def test_create_les_data32_and_io_arrays(ins, les_data32):
    data, files = les_data32
    assert len(data) == 2
    for d in data:
        assert d["u"].shape == (18, 18, 2, 5) and d["c"].shape == (18, 18, 2, 5) and d["u"].dtype == np.float32 and d["c"].dtype == np.float32
        assert np.isfinite(d["u"]).all() and np.isfinite(d["c"]).all() and np.abs(d["c"]).max() > 0
        assert d["t"].dtype == np.float64 and np.allclose(d["t"], [0.0, 0.003, 0.006, 0.009, 0.012])
    saved = np.load(files[1])
    assert saved["u"].dtype == np.float32 and saved["c"].dtype == np.float32
    assert np.array_equal(saved["u"], data[1]["u"]) and np.array_equal(saved["c"], data[1]["c"])
    les = ins.Setup(x=(axis(16), axis(16)), Re=1000.0)
    io = ins.create_io_arrays(data, les)
    for key in ("u", "c"):
        assert io[key].shape == (16, 16, 2, 10) and io[key].dtype == np.float32
        assert np.array_equal(io[key][..., :5], data[0][key][1:-1, 1:-1]) and np.array_equal(io[key][..., 5:], data[1][key][1:-1, 1:-1])


def test_create_les_data32_refuses_an_fp64_solver(ins):
    import torch

    with pytest.raises(TypeError, match="float32"):
        ins.create_les_data(D=2, Re=1000.0, lims=(0.0, 1.0), nles=[16], ndns=64, filters=(ins.FaceAverage(),), tburn=0.0, tsim=0.004, savefreq=2,
                            Δt=1e-3, rng=np.random.default_rng(0), dtype=torch.float32, create_psolver=ins.psolver_spectral)


# ------------------------------------------------------------------------------------ 4. training glue
def test_float32_training_glue(ins, les_data32):
    import torch

    f32, ad32 = ins.f32, ins.ad32
    n, dt, nstate = 32, 2e-3, 4
    sp = ins.Setup(x=(axis(n), axis(n)), Re=500.0)
    ps = f32.psolver_spectral32(sp)
    method = ins.RKMethods.RK44()
    u = f32.to_f32(sp, ins.random_field(sp, 0.0, psolver=ins.psolver_spectral(sp), seed=2))
    cache = f32.ERKCache32(method, sp, ps)
    us, ts = [ins.to_numpy(u)], [0.0]
    for k in range(nstate - 1):
        f32.timestep32_(cache, u, dt)
        us.append(1.01 * ins.to_numpy(u))  # perturbed reference: the error is not zero
        ts.append((k + 1) * dt)
    traj = dict(u=np.stack(us, axis=-1), t=np.array(ts))
    assert traj["u"].dtype == np.float32
    inner = (slice(1, -1), slice(1, -1))
    # a-posteriori error with a zero torch closure = the hand loop of ad32.timestep (F + 0 is exact)
    relerr = ins.create_relerr_post(data=traj, setup=sp, method=method, psolver=ps, closure_model=lambda v, θ: torch.zeros_like(v))
    e = relerr(None)
    U = torch.as_tensor(traj["u"], device=sp.device)
    with torch.no_grad():
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=f32.to_f32(sp, U[..., 0]), temp=None, t=0.0)
        want = 0.0
        for it in range(1, nstate):
            st = ad32.timestep(method, st, float(ts[it] - ts[it - 1]))
            assert st.u.dtype == torch.float32
            want += float(torch.linalg.vector_norm(st.u[inner] - U[..., it][inner]) / torch.linalg.vector_norm(U[..., it][inner]))
    print(f"Float32 relerr_post {e:.9e}, hand loop {want / (nstate - 1):.9e}")
    assert np.isfinite(e) and e > 0 and e == want / (nstate - 1)
    # a-posteriori loss through a float32 CNN: a float32 scalar with finite, non-zero parameter gradients
    m = ins.cnn(setup=sp, radii=[1, 1], channels=[4, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=3, dtype=torch.float32)
    loss = ins.create_loss_post(setup=sp, method=method, psolver=ps, closure_model=ins.wrappedclosure(m, sp))
    batch, _ = ins.create_dataloader_post([traj], ntrajectory=1, nunroll=nstate - 1, device=sp.device, dtype=torch.float32)(np.random.default_rng(0))
    assert batch[0]["u"].dtype == torch.float32
    val = loss(batch, None)
    assert val.dtype == torch.float32 and bool(torch.isfinite(val))
    grads = torch.autograd.grad(val, list(m.parameters()))
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    # a-priori training on float32 io arrays lowers the loss
    data, _ = les_data32
    les = ins.Setup(x=(axis(16), axis(16)), Re=1000.0)
    io = ins.create_io_arrays(data, les)
    m = ins.cnn(setup=les, radii=[2, 2], channels=[8, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=0, dtype=torch.float32)
    with torch.no_grad():
        m.convs[-1].weight.zero_()
    prior = ins.create_loss_prior(m)
    loader = ins.create_dataloader_prior((io["u"], io["c"]), batchsize=8, device=les.device, dtype=torch.float32)
    x, y = torch.as_tensor(io["u"], device=les.device), torch.as_tensor(io["c"], device=les.device)
    assert x.dtype == torch.float32
    with torch.no_grad():
        start = float(prior((x, y), None))
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    ins.train(dataloader=loader, loss=prior, trainstate=dict(opt=opt, θ=None, rng=np.random.default_rng(7)), niter=20)
    with torch.no_grad():
        final = prior((x, y), None)
    print(f"Float32 a-priori loss after 20 Adam iterations from the zero-output start: {float(final):.6f} (start {start})")
    assert final.dtype == torch.float32 and start == 1.0 and float(final) < start


# ------------------------------------------------------------------------------------ 5. the example
def test_neural_closure_2d_example_float32(ins):
    import torch

    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")
    sys.path.insert(0, ex)
    spec = importlib.util.spec_from_file_location("NeuralClosure2D", os.path.join(ex, "NeuralClosure2D.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    r = mod.main(ndns=64, nles=16, tsim=0.02, niter=10, verbose=False, dtype=torch.float32)
    assert r["u"].dtype == np.float32 and r["c"].dtype == np.float32
    assert r["u"].shape == (16, 16, 2, r["nsample"]) and r["c"].shape == r["u"].shape and r["nsample"] == 2 * 11
    for k in ("prior_before", "prior_after", "post_noclosure", "post_cnn"):
        assert np.isfinite(r[k]) and r[k] >= 0
    assert r["prior_before"] == 1.0
