"""GPU: the Float32 DNS-to-LES filter kernels (csrc/ins_filter32.hip) against the numpy restatement tests/filter_ref.py applied to the widened float
input, in double.

Tolerance.  The float kernels load floats, sum in double and round once at the store, so an output is the rounded value of a double result that
is itself within n·eps64·max|u| of the exact mean, and a mean is no larger than max|u|: |got − ref| ≤ ½ ulp32(max|u|) + n·eps64·max|u|
≤ eps32·max|u| (eps32 = 2⁻²³; n ≤ 9·64).  Nothing here is tuned to what the kernels give."""
import numpy as np
import pytest

from tests import filter_ref as fr
from tests import fixtures as fx
from tests.test_gpu_adjoint import mirror
from tests.test_gpu_filters import ANISO_CASES, PULLBACK_CASES, aniso, periodic, scatter_pullback, tiled_route

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = -7.25e3  # exact in float


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def randf32(ins, sp, seed):
    return ins.f32.to_f32(sp, fx.randn_field(tuple(sp.grid.N) + (sp.grid.dimension,), seed))


def wide(f):
    return np.asfortranarray(f.detach().cpu().numpy().astype(np.float64))


def filt(ins, kind):
    return ins.FaceAverage() if kind == "face" else ins.VolumeAverage()


def iu_mask(les, shape):
    mask = np.zeros(shape, dtype=bool)
    for a in range(les.grid.dimension):
        mask[tuple(slice(lo, hi) for lo, hi in les.grid.Iu[a]) + (a,)] = True
    return mask


def check_filter(ins, kind, les, dns, comp, seed=0):
    import torch

    u = randf32(ins, dns, seed)
    v = ins.f32.vectorfield32(les)
    v.fill_(SENTINEL)
    out = filt(ins, kind)(v, u, les, comp, setup_dns=dns)
    assert out is v and v.dtype == torch.float32
    got, un = wide(v), wide(u)
    ref = np.full_like(got, SENTINEL)
    if kind == "face":
        fr.face_average(un, les.grid.Iu, les.grid.N, comp, out=ref)
    else:
        fr.volume_average(un, tuple(n - 2 for n in les.grid.N), comp, out=ref)
    mask = iu_mask(les, got.shape)
    assert np.all(got[~mask] == SENTINEL), "values outside Iu were written"
    err, b = np.max(np.abs(got[mask] - ref[mask])), EPS32 * np.max(np.abs(un))
    print(f"f32 {kind} D={les.grid.dimension} comp={comp} N_les={les.grid.N}: max err {err:.3e}, bound {b:.3e}")
    assert err <= b
    return got


# ------------------------------------------------------------------------------------ 1. every value against the restatement
@pytest.mark.parametrize("comp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("D,n_les", [(2, 12), (3, 6)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_filters_match_restatement(ins, kind, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    check_filter(ins, kind, les, dns, comp, seed=comp)
    # the allocating form returns a float32 field
    import torch

    v = filt(ins, kind)(randf32(ins, dns, 1), les, comp, setup_dns=dns)
    assert v.dtype == torch.float32 and tuple(v.shape) == tuple(les.grid.N) + (D,)


# ------------------------------------------------------------------------------------ 2. reconstruct
@pytest.mark.parametrize("comp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("D,n_les", [(2, 12), (3, 6)])
def test_reconstruct_matches_restatement(ins, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    check_reconstruct(ins, les, dns, comp)


def check_reconstruct(ins, les, dns, comp):
    import torch

    v = ins.f32.apply_bc_u32_(randf32(ins, les, 5), les)
    u = ins.f32.vectorfield32(dns)
    u.fill_(SENTINEL)
    ins.reconstruct_(u, v, dns, les, comp)
    got, vn = wide(u), wide(v)
    ref = np.full_like(got, SENTINEL)
    fr.reconstruct(vn, tuple(n - 2 for n in les.grid.N), comp, out=ref)
    mask = np.zeros(got.shape, dtype=bool)
    mask[tuple(slice(1, n - 1) for n in dns.grid.N)] = True
    assert np.all(got[~mask] == SENTINEL), "reconstruct wrote outside the fine interior"
    vmax = np.max(np.abs(vn))
    assert np.max(np.abs(got[mask] - ref[mask])) <= EPS32 * vmax
    # FaceAverage(reconstruct(w)) == w: two roundings
    r = ins.reconstruct(v, dns, les, comp)
    assert r.dtype == torch.float32
    back = wide(ins.FaceAverage()(r, les, comp, setup_dns=dns))
    inner = tuple(slice(1, n - 1) for n in les.grid.N)
    assert np.max(np.abs(back[inner] - vn[inner])) <= 2 * EPS32 * vmax


# ------------------------------------------------------------------------------------ 3. wall-bounded, stretched and mixed-BC grids
@pytest.mark.parametrize("comp", [1, 2, 3])
@pytest.mark.parametrize("name", ["setup2d", "setup3d", "setup_mixed"])
def test_face_average_on_wall_bounded_and_stretched_grids(ins, oracle, name, comp):
    so = getattr(fx, name)(oracle)
    les = mirror(ins, so, oracle)
    xin = []
    for a in range(so.grid.D):
        lo = 2 if isinstance(so.boundary_conditions[a][0], oracle.PressureBC) else 1
        xin.append(fr.subdivide(so.grid.x[a][lo:-1], comp))
    dns = ins.Setup(x=xin, boundary_conditions=les.boundary_conditions, Re=so.Re)
    check_filter(ins, "face", les, dns, comp, seed=11)
    # the volume average and reconstruct need all-periodic grids
    lib, D = ins._lib.load(), les.grid.dimension
    u, v = ins.f32.vectorfield32(dns), ins.f32.vectorfield32(les)
    up, vp = ins.f32._ptr(dns, u, D), ins.f32._ptr(les, v, D)
    UNSUPPORTED = -4
    assert lib.ins_filter_volume_f32(les.handle, dns.handle, comp, up, vp, les.stream) == UNSUPPORTED
    assert lib.ins_filter_volume_pullback_f32(les.handle, dns.handle, comp, vp, up, les.stream) == UNSUPPORTED
    assert lib.ins_reconstruct_f32(dns.handle, les.handle, comp, vp, up, les.stream) == UNSUPPORTED
    with pytest.raises(ins.INSHipError):
        ins.VolumeAverage()(u, les, comp, setup_dns=dns)


# ------------------------------------------------------------------------------------ 4. tiled against generic
@pytest.mark.parametrize("n_dns,n_les", [(96, 48), (96, 24), (192, 48), (160, 20)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_tiled_matches_generic(ins, kind, n_dns, n_les):
    comp = n_dns // n_les
    les, dns = periodic(ins, n_les, 3), periodic(ins, n_dns, 3)
    check_tiled_matches_generic(ins, kind, les, dns, comp)


def check_tiled_matches_generic(ins, kind, les, dns, comp):
    u = randf32(ins, dns, 21)
    out = {}
    for off in (0, 1):
        with ins._lib.options(INS_DISABLE_FILTER_TILED=off):
            v = ins.f32.vectorfield32(les)
            v.fill_(SENTINEL)
            out[off] = filt(ins, kind)(v, u, les, comp, setup_dns=dns)
    inner = tuple(slice(1, n - 1) for n in les.grid.N)
    err = float((out[0].double() - out[1].double())[inner].abs().max())
    b = EPS32 * float(u.abs().max())
    print(f"f32 {kind} {tuple(dns.grid.N)} -> {tuple(les.grid.N)}: tiled - generic max {err:.3e}, bound {b:.3e}")
    assert err <= b
    for o in out.values():
        ghosts = o.clone()
        ghosts[inner] = SENTINEL
        assert bool((ghosts == SENTINEL).all())


# ------------------------------------------------------------------------------------ 4b. anisotropic boxes at the edges of the x tile
# The cases of tests/test_gpu_filters.py (the fp64 tile of 64 fine x-volumes) and the float tile of 128 (two volumes per lane).
ANISO32_CASES = ANISO_CASES + [
    (4, (32, 5, 2)),  # n_dns0 = 128: exactly one float tile, the x halo of the last volume-average output wraps to fine index 1
    (8, (17, 3, 2)),  # 136: a tile plus one coarse output
    (2, (68, 5, 3)),  # 136: the float face average at comp 2 is tiled
]


@pytest.mark.parametrize("comp,n_les", ANISO32_CASES)
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_anisotropic_tile_edges_match_restatement(ins, kind, comp, n_les):
    les, dns = aniso(ins, comp, n_les)
    got = check_filter(ins, kind, les, dns, comp, seed=40 + comp)
    with ins._lib.options(INS_DISABLE_FILTER_TILED=1):
        generic = check_filter(ins, kind, les, dns, comp, seed=40 + comp)
    if tiled_route(kind, comp, face2=True):
        check_tiled_matches_generic(ins, kind, les, dns, comp)
    else:  # the switch must change nothing where no tiled kernel serves
        assert np.array_equal(got, generic)


@pytest.mark.parametrize("comp,n_les", [(c, n) for c, n in ANISO32_CASES if c in (3, 4)])
def test_reconstruct_on_anisotropic_boxes(ins, comp, n_les):
    les, dns = aniso(ins, comp, n_les)
    check_reconstruct(ins, les, dns, comp)


# ------------------------------------------------------------------------------------ 5. transposes
def check_transpose32(Φu, w, u, ΦTw):
    """The dot products on the host in double from the float arrays; every stored value carries at most half an ulp, then Cauchy-Schwarz."""
    Φu, w, u, ΦTw = wide(Φu), wide(w), wide(u), wide(ΦTw)
    lhs, rhs = float(np.sum(Φu * w)), float(np.sum(u * ΦTw))
    b = EPS32 * (np.linalg.norm(Φu) * np.linalg.norm(w) + np.linalg.norm(u) * np.linalg.norm(ΦTw))
    print(f"<Φu, w> = {lhs:.9e}, <u, Φᵀw> = {rhs:.9e}, diff {abs(lhs - rhs):.3e}, bound {b:.3e}")
    assert b > 0 and abs(lhs - rhs) <= b


@pytest.mark.parametrize("comp", [1, 2, 3, 4])
@pytest.mark.parametrize("D,n_les", [(2, 8), (3, 4)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_pullbacks_are_transposes(ins, kind, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    Φ = filt(ins, kind)
    u, w = randf32(ins, dns, 1), randf32(ins, les, 2)
    Φu = Φ(u, les, comp, setup_dns=dns)  # zeros outside Iu
    ΦTw = ins.f32.vectorfield32(dns)
    ΦTw.fill_(SENTINEL)  # the pullback overwrites the whole padded array
    Φ.pullback_(ΦTw, w, les, comp, dns)
    assert not bool((ΦTw == SENTINEL).any())
    check_transpose32(Φu, w, u, ΦTw)
    if kind == "face":  # zeros where the forward reads nothing: the fine ghost layers
        g = wide(ΦTw)
        g[tuple(slice(1, n - 1) for n in dns.grid.N)] = 0.0
        assert not g.any()


PULLBACK32_CASES = PULLBACK_CASES + [(c, n) for c, n in ANISO32_CASES[len(ANISO_CASES):] if c in (2, 4)]


@pytest.mark.parametrize("comp,n_les", PULLBACK32_CASES)
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_pullbacks_match_scatter_restatement(ins, kind, comp, n_les):
    """Every value of the whole padded fine cotangent against the scatter restatement applied to the widened float cotangent, in double: the gather
    is summed in double and rounded once at the store, and no value exceeds max|w|, so the bound of this file holds."""
    les, dns = aniso(ins, comp, n_les)
    w = randf32(ins, les, 50 + comp)  # non-zero in the coarse ghost volumes
    ΦTw = ins.f32.vectorfield32(dns)
    ΦTw.fill_(SENTINEL)
    filt(ins, kind).pullback_(ΦTw, w, les, comp, dns)
    got, wn = wide(ΦTw), wide(w)
    ref = scatter_pullback(kind, wn, les, dns, comp)
    err, b = np.max(np.abs(got - ref)), EPS32 * np.max(np.abs(wn))
    print(f"f32 {kind} pullback D={len(n_les)} comp={comp} N_les={tuple(les.grid.N)}: max err {err:.3e}, bound {b:.3e}")
    assert np.max(np.abs(ref)) > 0 and err <= b


def test_face_pullback_on_mixed_bc_grid(ins, oracle):
    les = mirror(ins, fx.setup_mixed(oracle), oracle)
    dns = ins.neuralclosure.dns_setup_of(les, 2)
    Φ = ins.FaceAverage()
    u, w = randf32(ins, dns, 1), randf32(ins, les, 2)
    Φu = Φ(u, les, 2, setup_dns=dns)
    ΦTw = ins.f32.vectorfield32(dns)
    ΦTw.fill_(SENTINEL)
    Φ.pullback_(ΦTw, w, les, 2, dns)
    assert not bool((ΦTw == SENTINEL).any())
    check_transpose32(Φu, w, u, ΦTw)


# ------------------------------------------------------------------------------------ 6. autograd
@pytest.mark.parametrize("D,n_les,comp", [(2, 8, 2), (3, 4, 3)])
@pytest.mark.parametrize("kind", ["FaceAverage", "VolumeAverage"])
def test_ad32_filters(ins, kind, D, n_les, comp):
    import torch

    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    Φ = getattr(ins, kind)()
    u, w = randf32(ins, dns, 9).requires_grad_(True), randf32(ins, les, 10)
    v = getattr(ins.ad32, kind).apply(u, les, comp, dns)
    assert v.dtype == torch.float32 and bool((v == Φ(u.detach(), les, comp, setup_dns=dns)).all())
    (v * w).sum().backward()
    ref = Φ.pullback_(ins.f32.vectorfield32(dns), w, les, comp, dns)
    assert u.grad.dtype == torch.float32 and bool((u.grad == ref).all())
    with pytest.raises(TypeError):
        getattr(ins.ad32, kind).apply(u.detach().double(), les, comp, dns)


# ------------------------------------------------------------------------------------ 7. apply_bc_u32_(dudt=True)
@pytest.mark.parametrize("case", ["setup3d", "lid2d"])
def test_apply_bc_u32_dudt(ins, oracle, case):
    """With `dudt` the Dirichlet data term is zero and every ghost formula is a copy or a zero (k_bc_u, ins_operator_kernels.h): no side rounds,
    so the widened float result is the fp64 result of the widened input exactly."""
    if case == "setup3d":
        sp = mirror(ins, fx.setup3d(oracle), oracle)
    else:
        ax = np.linspace(0.0, 1.0, 13)
        lid = (ins.DirichletBC(), ins.DirichletBC((1.5, 0.25)))
        sp = ins.Setup(x=(ax, ax), boundary_conditions=((ins.DirichletBC(), ins.DirichletBC()), lid), Re=1000.0)
    u = randf32(ins, sp, 4)
    ref = ins.apply_bc_u_(u.double(), 0.3, sp, dudt=True)
    plain = ins.f32.apply_bc_u32_(u.clone(), sp)
    got = ins.f32.apply_bc_u32_(u.clone(), sp, dudt=True)
    assert bool((got.double() == ref).all())
    if case == "lid2d":  # the lid value enters without dudt only
        assert bool((plain.double() == ins.apply_bc_u_(u.double(), 0.3, sp)).all())
        assert not bool((plain == got).all())
