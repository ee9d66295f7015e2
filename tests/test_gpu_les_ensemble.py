"""Ensemble filtered-DNS data on the device: `ensemble_rhs_` (csrc/ins_rk_ensemble.hip), the member filters `Φ.members` (k_filter_members,
csrc/ins_filter_kernels.h) and `create_les_data_ensemble`.

  * per member the new entries are BITWISE what they give for that field alone (B = 1), and the member filters bitwise `Φ(v, u, …)`: the member is one more
    launch dimension of the same text;
  * against the public per-member chain `apply_bc_u_(project_(apply_bc_u_(momentum_(…), dudt=True)))` the right-hand side agrees to POISSON_TOL (1e-11
    relative L2, the tolerance of this chain in tests/test_gpu_parity.py): the fused kernels sum in another order, so this check is not bitwise;
  * `create_les_data_ensemble` against consecutive `create_les_data` calls with an identically seeded rng: `u` and `t` bitwise, `c` to POISSON_TOL.

Boxes of the right-hand side: 16 x 32 (one-launch solve), 64 x 64 (two x tiles), 128 x 16 (three-pass solve), those of tests/test_gpu_ensemble.py.
Filter shapes: 64 x 32 -> 32 x 16 (comp 2), 64 x 64 -> 16 x 16 (comp 4), 48 x 24 -> 16 x 8 (comp 3: the odd volume window)."""
import numpy as np
import pytest
import torch

from tests import filter_ref as fr
from tests import fixtures as fx
from tests.test_gpu_parity import OP_TOL, POISSON_TOL

pytestmark = pytest.mark.gpu

GRIDS = [(16, 32), (64, 64), (128, 16)]
BS = (1, 3, 7)
SENTINEL = -7.25
PAD = 5  # elements between two members in the padded layouts


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def rell2(a, b):
    return float(np.sqrt(np.sum((a - b) ** 2)) / np.sqrt(np.sum(b**2)))


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _setup(ins, n, Re=500.0):
    return ins.Setup(x=tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n), Re=Re, device="cuda:0")


def _divfree(ins, sp, ps, seed):
    u = ins.from_numpy(sp, 0.3 * fx.randn_field(sp.grid.N + (2,), seed))
    ins.apply_bc_u_(u, 0.0, sp)
    ins.project_(u, sp, ps, ins.scalarfield(sp))
    return ins.apply_bc_u_(u, 0.0, sp)


def _padded(sp, B, fill=SENTINEL):
    """B members in the layout of `vectorfields` with PAD sentinel elements behind every member: (view of the members, the flat buffer, elements per member)."""
    shape = sp.grid.N + (2,)
    m = int(np.prod(shape))
    flat = torch.full((B * (m + PAD),), fill, dtype=torch.float64, device=sp.device)
    strides = (m + PAD,) + tuple(int(np.prod(shape[:q])) for q in range(len(shape)))
    return flat.as_strided((B,) + shape, strides), flat, m


def _pads(flat, B, m):
    return flat.view(B, m + PAD)[:, m:]


def _chain(ins, sp, ps, u):
    """The public per-member chain that `ensemble_rhs_` replaces."""
    F = ins.momentum_(ins.vectorfield(sp), u, None, 0.0, sp)
    ins.apply_bc_u_(F, 0.0, sp, dudt=True)
    ins.project_(F, sp, ps, ins.scalarfield(sp))
    return ins.apply_bc_u_(F, 0.0, sp)


# ------------------------------------------------------------------------------------------------ ensemble_rhs_
@pytest.mark.parametrize("n", GRIDS)
def test_ensemble_rhs(ins, n):
    sp = _setup(ins, n)
    ps = ins.psolver_spectral(sp)
    rk44 = ins.RKMethods.RK44()
    starts = [_divfree(ins, sp, ps, 20 + b) for b in range(max(BS))]
    starts[2].zero_()  # a zero member
    # the single-field state of the solver and a live ERKCache, before
    live = ins.ode_method_cache(rk44, sp, ps)

    def alone():
        u = ins.copyfield(starts[0])
        ins.timesteps_(rk44, ins.create_stepper(rk44, setup=sp, psolver=ps, u=u), 2e-3, 2, cache=live)
        return u

    before = alone()
    one = ins.EnsembleCache(rk44, sp, ps, 1)
    want = []
    for u0 in starts:  # B = 1 on every field alone: once, shared by every B
        U1 = ins.vectorfields(sp, 1)
        U1[0].copy_(u0)
        want.append(ins.ensemble_rhs_(one, ins.vectorfields(sp, 1), U1)[0].clone())
    assert not torch.equal(want[0], want[1]) and float(want[0].abs().max()) > 0
    assert float(want[2].abs().max()) == 0.0  # a zero member gives zero
    perm = [3, 0, 6, 1, 5, 2, 4]
    for B in BS:
        cache = ins.EnsembleCache(rk44, sp, ps, B)
        U, uflat, m = _padded(sp, B)
        F, fflat, _ = _padded(sp, B)
        for b in range(B):
            U[b].copy_(starts[b])
        keep = uflat.clone()
        assert ins.ensemble_rhs_(cache, F, U) is F
        assert torch.equal(uflat, keep)  # U unchanged bitwise, its padding included
        assert bool((_pads(fflat, B, m) == SENTINEL).all())  # the pad between members of F is untouched
        for b in range(B):
            assert torch.equal(F[b], want[b]), (n, B, b, float((F[b] - want[b]).abs().max()))
            got, ref = ins.to_numpy(F[b]), ins.to_numpy(_chain(ins, sp, ps, starts[b]))
            if b != 2:
                e = rell2(got, ref)
                print(f"rhs {n} B={B} member {b}: rell2 vs per-member chain {e:.3e}")
                assert e < POISSON_TOL
            else:
                assert not ref.any()
        if B == 7:  # a permutation of members permutes the result
            Up = ins.vectorfields(sp, B)
            for b in range(B):
                Up[b].copy_(starts[perm[b]])
            Fp = ins.ensemble_rhs_(cache, ins.vectorfields(sp, B), Up)
            for b in range(B):
                assert torch.equal(Fp[b], want[perm[b]])
            with pytest.raises(ValueError):
                ins.ensemble_rhs_(cache, Up, Up)
    assert torch.equal(alone(), before)  # the solver's single-field state and the live cache are as they were


def test_ensemble_apply_bc_u(ins):
    sp = _setup(ins, (16, 32))
    ps = ins.psolver_spectral(sp)
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, 3)
    U, flat, m = _padded(sp, 3)
    for b in range(3):
        U[b].copy_(ins.from_numpy(sp, fx.randn_field(sp.grid.N + (2,), b)))
    want = [ins.apply_bc_u(U[b], 0.0, sp) for b in range(3)]
    ins.ensemble_apply_bc_u_(cache, U)
    assert all(torch.equal(U[b], want[b]) for b in range(3)) and bool((_pads(flat, 3, m) == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ member filters
@pytest.mark.parametrize("nf, comp", [((64, 32), 2), ((64, 64), 4), ((48, 24), 3)])
def test_member_filters(ins, nf, comp):
    ncs = tuple(q // comp for q in nf)
    dns, les = _setup(ins, nf), _setup(ins, ncs)
    fine = [ins.from_numpy(dns, fx.randn_field(dns.grid.N + (2,), 40 + b)) for b in range(max(BS))]
    for Φ, name in ((ins.FaceAverage(), "face"), (ins.VolumeAverage(), "volume")):
        want = []
        for u in fine:  # the single-field filter into a sentinel field: once, shared by every B
            v = ins.vectorfield(les)
            v.fill_(SENTINEL)
            want.append(Φ(v, u, les, comp, setup_dns=dns))
        href = fr.face_average(ins.to_numpy(fine[0]), les.grid.Iu, les.grid.N, comp) if name == "face" else fr.volume_average(ins.to_numpy(fine[0]), ncs, comp)
        for B in BS:
            U, _, _ = _padded(dns, B)
            V, vflat, m = _padded(les, B)
            for b in range(B):
                U[b].copy_(fine[b])
            assert Φ.members(V, U, les, comp, setup_dns=dns) is V
            for b in range(B):
                assert torch.equal(V[b], want[b]), (name, nf, comp, B, b)  # bitwise Φ(v, u, …), coarse ghosts still the sentinel
            assert bool((_pads(vflat, B, m) == SENTINEL).all())
            g = ins.to_numpy(V[0])
            assert (g[0] == SENTINEL).all() and (g[-1] == SENTINEL).all() and (g[:, 0] == SENTINEL).all() and (g[:, -1] == SENTINEL).all()
            for a in range(2):
                sl = tuple(slice(lo, hi) for lo, hi in les.grid.Iu[a])
                e = relmax(g[sl + (a,)], href[sl + (a,)])
                assert e < OP_TOL, (name, nf, comp, B, a, e)
        with pytest.raises(ValueError):
            Φ.members(ins.vectorfields(les, 2), ins.vectorfields(dns, 3), les, comp, setup_dns=dns)


# ------------------------------------------------------------------------------------------------ create_les_data_ensemble
def _compare(ins, ens, seq, nles):
    """`ens[b][pair]` against `seq[b][pair]`: shapes and order, u and t bitwise, c to POISSON_TOL over the interior."""
    assert len(ens) == len(seq)
    worst = 0.0
    for eb, sb in zip(ens, seq):
        assert len(eb) == len(sb)
        for e, s in zip(eb, sb):
            assert sorted(e) == sorted(s) == ["c", "comptime", "t", "u"]
            assert e["u"].shape == s["u"].shape and e["c"].shape == s["c"].shape and e["u"].dtype == s["u"].dtype
            assert np.array_equal(e["u"], s["u"]) and np.array_equal(e["t"], s["t"])
            for it in range(len(s["t"])):
                err = rell2(e["c"][1:-1, 1:-1, :, it], s["c"][1:-1, 1:-1, :, it])
                worst = max(worst, err)
                assert err < POISSON_TOL, err
    print(f"create_les_data_ensemble: worst rell2 of c against per-seed create_les_data {worst:.3e}")


def test_create_les_data_ensemble(ins, tmp_path):
    kw = dict(D=2, Re=1000.0, lims=(0.0, 1.0), nles=(16, 32), ndns=64, filters=(ins.FaceAverage(), ins.VolumeAverage()), tburn=0.004, tsim=0.012,
              savefreq=3, Δt=1e-3)
    B = 3
    rng = np.random.default_rng(0)
    seq = [ins.create_les_data(rng=rng, **kw) for _ in range(B)]
    files = [[str(tmp_path / f"m{b}_{q}.npz") for q in range(4)] for b in range(B)]
    ens = ins.create_les_data_ensemble(ntrajectory=B, rng=np.random.default_rng(0), filenames=files, **kw)
    assert len(ens) == B and len(ens[0]) == 4 and ens[0][0]["u"].shape == (18, 18, 2, 5) and ens[0][1]["u"].shape == (34, 34, 2, 5)
    assert np.array_equal(ens[0][0]["t"], seq[0][0]["t"]) and len(ens[0][0]["t"]) == 5
    assert not np.array_equal(ens[0][0]["u"], ens[1][0]["u"])
    _compare(ins, ens, seq, kw["nles"])
    for b in range(B):  # files reload equal
        for q in range(4):
            saved = np.load(files[b][q])
            assert np.array_equal(saved["u"], ens[b][q]["u"]) and np.array_equal(saved["c"], ens[b][q]["c"]) and np.array_equal(saved["t"], ens[b][q]["t"])
    # create_io_arrays on the concatenated trajectories of one (filter, grid) pair
    for q, n in ((0, 16), (1, 32), (2, 16), (3, 32)):
        les = _setup(ins, (n, n), Re=1000.0)
        ie, iseq = ins.create_io_arrays([ens[b][q] for b in range(B)], les), ins.create_io_arrays([seq[b][q] for b in range(B)], les)
        assert ie["u"].shape == (n, n, 2, 5 * B) and np.array_equal(ie["u"], iseq["u"])
        assert ie["c"].shape == iseq["c"].shape and rell2(ie["c"], iseq["c"]) < POISSON_TOL
    # the trajectories feed the a-posteriori loader unchanged
    loader = ins.create_dataloader_post([ens[b][0] for b in range(B)], ntrajectory=2, nunroll=2, device="cuda:0")
    batch, _ = loader(np.random.default_rng(1))
    assert len(batch) == 2 and tuple(batch[0]["u"].shape) == (18, 18, 2, 3)


def test_create_les_data_ensemble_three_pass_dns(ins):
    """ndns = 128: the DNS solve takes its three-pass route; two saves (the initial state and one more), a shorter last batch is stepped and not saved."""
    kw = dict(D=2, Re=1000.0, lims=(0.0, 1.0), nles=(32,), ndns=128, filters=(ins.FaceAverage(), ins.VolumeAverage()), tburn=0.002, tsim=0.003,
              savefreq=2, Δt=1e-3)
    rng = np.random.default_rng(3)
    seq = [ins.create_les_data(rng=rng, **kw) for _ in range(2)]
    ens = ins.create_les_data_ensemble(ntrajectory=2, rng=np.random.default_rng(3), **kw)
    assert len(seq[0][0]["t"]) == 2 and ens[0][0]["u"].shape == (34, 34, 2, 2)
    _compare(ins, ens, seq, kw["nles"])


# ------------------------------------------------------------------------------------------------ refusals that need the device
def test_device_side_refusals(ins):
    # a 3-D filter call
    les3, dns3 = _setup(ins, (4, 4, 4)), _setup(ins, (8, 8, 8))
    U, V = ins.vectorfields(dns3, 2), ins.vectorfields(les3, 2)
    for Φ, entry in ((ins.FaceAverage(), "ins_filter_face_f64"), (ins.VolumeAverage(), "ins_filter_volume_f64")):
        with pytest.raises(NotImplementedError) as e:
            Φ.members(V, U, les3, 2, setup_dns=dns3)
        assert entry in str(e.value) and "V[b], U[b], setup_les, comp" in str(e.value) and "3-D" in str(e.value)
    assert not bool(V.any())
    # a cache whose box an option has since switched off
    sp = _setup(ins, (32, 32))
    ps = ins.psolver_spectral(sp)
    cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, 2)
    U, F = ins.vectorfields(sp, 2), ins.vectorfields(sp, 2)
    U[0].copy_(_divfree(ins, sp, ps, 1))
    lib = ins._lib.load()
    assert lib.ins_set_option(b"INS_DISABLE_CORR2D", 1) == 0
    try:
        with pytest.raises(NotImplementedError) as e:
            ins.ensemble_rhs_(cache, F, U)
        assert "ins_project_f64" in str(e.value) and "per member" in str(e.value) and "switched" in str(e.value)
        with pytest.raises(NotImplementedError) as e:
            ins.ensemble_apply_bc_u_(cache, U)
        assert "per member" in str(e.value)
    finally:
        assert lib.ins_set_option(b"INS_DISABLE_CORR2D", 0) == 0
    assert not bool(F.any())
    assert bool(ins.ensemble_rhs_(cache, F, U)[0].any())
