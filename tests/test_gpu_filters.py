"""GPU: the DNS-to-LES filter kernels (csrc/ins_filter.hip) through the C ABI, against the numpy restatement tests/filter_ref.py.

Tolerance.  A mean of n terms summed in one order differs from the same mean summed in another order by at most 2·n·eps·max|u|
(each of the ≤ n − 1 additions of either order rounds a partial sum of magnitude ≤ n·max|u| by eps/2, then one division): n = comp^(D−1)
for the face average, (comp + 1)·comp^(D−1) for the volume average.  Nothing here is tuned to what the kernels give.

Shapes.  Cubes with one spacing hide a swap of two directions, so section 3b repeats the value-by-value checks on boxes with three different sizes
and lengths whose fine width sits at the edges of the 64-wide x tile, and section 4 checks every value of the pullbacks and of reconstruct there
against the scatter restatements of tests/filter_ref.py (pinned to the dense transposes by tests/test_filters_cpu.py)."""
import numpy as np
import pytest

from tests import filter_ref as fr
from tests import fixtures as fx
from tests.test_gpu_adjoint import TOL, dot, mirror, nrm

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SENTINEL = -7.25e3


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def periodic(ins, n, D, L=1.0):
    """`n` and `L`: one value for every direction, or one per direction."""
    n = (n,) * D if isinstance(n, int) else tuple(n)
    L = (L,) * D if isinstance(L, (int, float)) else tuple(L)
    assert len(n) == D and len(L) == D
    return ins.Setup(x=tuple(np.linspace(0.0, Li, ni + 1) for ni, Li in zip(n, L)), Re=1000.0)


def randf(ins, sp, seed):
    return ins.from_numpy(sp, fx.randn_field(tuple(sp.grid.N) + (sp.grid.dimension,), seed))


def bound(nterms, umax):
    return 2 * nterms * EPS * umax


def nterms(kind, comp, D):
    return comp ** (D - 1) * ((comp + 1 if comp % 2 == 0 else comp) if kind == "volume" else 1)


def check_filter(ins, kind, les, dns, comp, seed=0):
    D = les.grid.dimension
    u = randf(ins, dns, seed)
    v = ins.vectorfield(les)
    v.fill_(SENTINEL)
    Φ = ins.FaceAverage() if kind == "face" else ins.VolumeAverage()
    Φ(v, u, les, comp, setup_dns=dns)
    got, un = ins.to_numpy(v), ins.to_numpy(u)
    ref = np.full_like(got, SENTINEL)
    if kind == "face":
        fr.face_average(un, les.grid.Iu, les.grid.N, comp, out=ref)
    else:
        fr.volume_average(un, tuple(n - 2 for n in les.grid.N), comp, out=ref)
    mask = np.zeros(got.shape, dtype=bool)
    for a in range(D):
        mask[tuple(slice(lo, hi) for lo, hi in les.grid.Iu[a]) + (a,)] = True
    assert np.all(got[~mask] == SENTINEL), "values outside Iu were written"
    err = np.max(np.abs(got[mask] - ref[mask]))
    b = bound(nterms(kind, comp, D), np.max(np.abs(un)))
    print(f"{kind} D={D} comp={comp} N_les={les.grid.N}: max err {err:.3e}, bound {b:.3e}")
    assert err <= b
    return got


# ------------------------------------------------------------------------------------ 1. every value against the restatement
@pytest.mark.parametrize("comp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("D,n_les", [(2, 12), (3, 6)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_filters_match_restatement(ins, kind, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    check_filter(ins, kind, les, dns, comp, seed=comp)


def check_reconstruct(ins, les, dns, comp):
    v = ins.apply_bc_u(randf(ins, les, 5), 0.0, les)
    u = ins.vectorfield(dns)
    u.fill_(SENTINEL)
    ins.reconstruct_(u, v, dns, les, comp)
    got = ins.to_numpy(u)
    ref = np.full_like(got, SENTINEL)
    fr.reconstruct(ins.to_numpy(v), tuple(n - 2 for n in les.grid.N), comp, out=ref)
    inner = tuple(slice(1, n - 1) for n in dns.grid.N)
    mask = np.zeros(got.shape, dtype=bool)
    mask[inner] = True
    assert np.all(got[~mask] == SENTINEL)
    # two products and one sum of terms ≤ comp·max|v|, then a division: well inside 2·2·eps·max|v|·comp / comp
    assert np.max(np.abs(got[mask] - ref[mask])) <= bound(2, np.max(np.abs(ins.to_numpy(v))))


@pytest.mark.parametrize("comp", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("D,n_les", [(2, 12), (3, 6)])
def test_reconstruct_matches_restatement(ins, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    check_reconstruct(ins, les, dns, comp)


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
    # the fine grid the filter builds on its own is the same one
    u = randf(ins, dns, 12)
    a, b = ins.FaceAverage()(u, les, comp), ins.FaceAverage()(u, les, comp, setup_dns=dns)
    assert bool((a == b).all())


# ------------------------------------------------------------------------------------ 2. the identities of tests/test_filters_cpu.py on the device
@pytest.mark.parametrize("D,n_les,comp", [(2, 64, 2), (2, 64, 3), (3, 32, 2), (3, 32, 4)])
def test_identities_on_device(ins, D, n_les, comp):
    import torch

    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    inner_l = tuple(slice(1, n - 1) for n in les.grid.N)
    # constants are preserved
    c = ins.vectorfield(dns)
    c.fill_(3.83)
    for Φ in (ins.FaceAverage(), ins.VolumeAverage()):
        v = Φ(c, les, comp, setup_dns=dns)
        assert float((v[inner_l] - 3.83).abs().max()) <= 4 * EPS * 3.83
    # the face average of a divergence-free field is divergence-free
    ps = ins.psolver_spectral(dns)
    u = ins.apply_bc_u(randf(ins, dns, 7), 0.0, dns)
    u = ins.apply_bc_u_(ins.project_(u, dns, ps, ins.scalarfield(dns)), 0.0, dns)
    div_dns = ins.max_abs_divergence(u, dns)
    v = ins.apply_bc_u_(ins.FaceAverage()(u, les, comp, setup_dns=dns), 0.0, les)
    div_les = ins.max_abs_divergence(v, les)
    print(f"D={D} n_les={n_les} comp={comp}: max|div| DNS {div_dns:.3e} LES {div_les:.3e}")
    assert div_les <= 10 * div_dns
    # FaceAverage(reconstruct(w)) == w
    w = ins.apply_bc_u(randf(ins, les, 3), 0.0, les)
    back = ins.FaceAverage()(ins.reconstruct(w, dns, les, comp), les, comp, setup_dns=dns)
    assert float((back - w)[inner_l].abs().max()) <= 4 * EPS * float(w.abs().max())
    del ps
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ 3. tiled against generic
@pytest.mark.parametrize("n_dns,n_les", [(256, 128), (256, 64), (256, 32), (96, 48)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_tiled_matches_generic(ins, kind, n_dns, n_les):
    comp = n_dns // n_les
    les, dns = periodic(ins, n_les, 3), periodic(ins, n_dns, 3)
    check_tiled_matches_generic(ins, kind, les, dns, comp)


def check_tiled_matches_generic(ins, kind, les, dns, comp):
    u = randf(ins, dns, 21)
    Φ = ins.FaceAverage() if kind == "face" else ins.VolumeAverage()
    out = {}
    for off in (0, 1):
        with ins._lib.options(INS_DISABLE_FILTER_TILED=off):
            v = ins.vectorfield(les)
            v.fill_(SENTINEL)
            out[off] = Φ(v, u, les, comp, setup_dns=dns)
    inner = tuple(slice(1, n - 1) for n in les.grid.N)
    err = float((out[0] - out[1])[inner].abs().max())
    b = bound(nterms(kind, comp, 3), float(u.abs().max()))
    print(f"{kind} {tuple(dns.grid.N)} -> {tuple(les.grid.N)}: tiled - generic max {err:.3e}, bound {b:.3e}")
    assert err <= b
    ghosts = out[0].clone()
    ghosts[inner] = SENTINEL
    assert bool((ghosts == SENTINEL).all())
    return out


@pytest.mark.parametrize("case", ["odd_comp", "two_d", "walls"])
def test_sizes_the_tiled_kernel_refuses(ins, oracle, case):
    if case == "odd_comp":
        les, dns, comp = periodic(ins, 16, 3), periodic(ins, 48, 3), 3
    elif case == "two_d":
        les, dns, comp = periodic(ins, 32, 2), periodic(ins, 128, 2), 4
    else:
        les = mirror(ins, fx.setup3d(oracle), oracle)
        comp = 2
        dns = ins.neuralclosure.dns_setup_of(les, comp)
    ref = check_filter(ins, "face", les, dns, comp, seed=31)
    with ins._lib.options(INS_DISABLE_FILTER_TILED=1):
        again = check_filter(ins, "face", les, dns, comp, seed=31)
    assert np.array_equal(ref, again)


# ------------------------------------------------------------------------------------ 3b. anisotropic boxes at the edges of the x tile
# Three different sizes and three different lengths per box, so a y / z swap of a wrap length, a stride or a window changes the result.  The fp64
# tile is 64 fine x-volumes (the Float32 one 128, tests/test_gpu_filters32.py).  (comp, n_les): n_dns = comp · n_les.
ANISO_L = (1.0, 0.7, 1.9)
ANISO_CASES = [
    (8, (8, 5, 2)),   # n_dns0 = 64: exactly one tile, the x halo of the last volume-average output wraps to fine index 1; 4 + 1 coarse rows
    (8, (9, 3, 3)),   # 72: a tile plus one coarse output
    (4, (18, 5, 3)),  # 72: a tile plus two outputs
    (2, (36, 5, 3)),  # comp 2: the volume average is tiled, the fp64 face average generic
    (3, (24, 5, 3)),  # odd comp: the generic kernel across an x seam of its 64-wide launch
]


def aniso(ins, comp, n_les):
    D = len(n_les)
    return periodic(ins, n_les, D, ANISO_L[:D]), periodic(ins, tuple(comp * n for n in n_les), D, ANISO_L[:D])


def tiled_route(kind, comp, D=3, face2=False):
    """csrc/ins_filter_kernels.h tiled_supported: `face2` is the Float32 face average at comp 2."""
    return D == 3 and (comp in (4, 8) or (comp == 2 and (kind == "volume" or face2)))


@pytest.mark.parametrize("comp,n_les", ANISO_CASES)
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_anisotropic_tile_edges_match_restatement(ins, kind, comp, n_les):
    les, dns = aniso(ins, comp, n_les)
    assert tuple(dns.grid.N) == tuple(comp * n + 2 for n in n_les)
    got = check_filter(ins, kind, les, dns, comp, seed=40 + comp)
    with ins._lib.options(INS_DISABLE_FILTER_TILED=1):
        generic = check_filter(ins, kind, les, dns, comp, seed=40 + comp)
    if tiled_route(kind, comp):
        check_tiled_matches_generic(ins, kind, les, dns, comp)
    else:  # the switch must change nothing where no tiled kernel serves
        assert np.array_equal(got, generic)


# ------------------------------------------------------------------------------------ 4. transposes and autograd
@pytest.mark.parametrize("comp", [1, 2, 3, 4])
@pytest.mark.parametrize("D,n_les", [(2, 8), (3, 4)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_pullbacks_are_transposes(ins, kind, D, n_les, comp):
    les, dns = periodic(ins, n_les, D), periodic(ins, n_les * comp, D)
    Φ = ins.FaceAverage() if kind == "face" else ins.VolumeAverage()
    u, w = randf(ins, dns, 1), randf(ins, les, 2)
    Φu = Φ(u, les, comp, setup_dns=dns)
    ΦTw = ins.vectorfield(dns)
    ΦTw.fill_(SENTINEL)  # the pullback overwrites the whole padded array
    Φ.pullback_(ΦTw, w, les, comp, dns)
    lhs, rhs = dot(Φu, w), dot(u, ΦTw)
    assert abs(lhs - rhs) <= TOL * nrm(Φu) * nrm(w), (lhs, rhs)


PULLBACK_CASES = [(c, n) for c, n in ANISO_CASES if c in (2, 3, 4)] + [(4, (33, 5))]  # 2-D: n_dns0 = 132, three x tiles of the 64-wide launch


def scatter_pullback(kind, wn, les, dns, comp):
    if kind == "face":
        return fr.face_average_pullback(wn, les.grid.Iu, dns.grid.N, comp)
    return fr.volume_average_pullback(wn, tuple(n - 2 for n in les.grid.N), comp)


@pytest.mark.parametrize("comp,n_les", PULLBACK_CASES)
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_pullbacks_match_scatter_restatement(ins, kind, comp, n_les):
    """Every value of the whole padded fine cotangent.  A fine volume receives at most nterms / comp^D ≤ nterms contributions w / count, so the
    bound of a sum of nterms terms of size max|w| holds."""
    les, dns = aniso(ins, comp, n_les)
    D = len(n_les)
    Φ = ins.FaceAverage() if kind == "face" else ins.VolumeAverage()
    w = randf(ins, les, 50 + comp)  # non-zero in the coarse ghost volumes
    ΦTw = ins.vectorfield(dns)
    ΦTw.fill_(SENTINEL)  # the pullback overwrites the whole padded array
    Φ.pullback_(ΦTw, w, les, comp, dns)
    got, wn = ins.to_numpy(ΦTw), ins.to_numpy(w)
    ref = scatter_pullback(kind, wn, les, dns, comp)
    err, b = np.max(np.abs(got - ref)), bound(nterms(kind, comp, D), np.max(np.abs(wn)))
    print(f"{kind} pullback D={D} comp={comp} N_les={tuple(les.grid.N)}: max err {err:.3e}, bound {b:.3e}")
    assert np.max(np.abs(ref)) > 0 and err <= b


@pytest.mark.parametrize("comp,n_les", [(c, n) for c, n in ANISO_CASES if c in (3, 4)])
def test_reconstruct_on_anisotropic_boxes(ins, comp, n_les):
    les, dns = aniso(ins, comp, n_les)
    check_reconstruct(ins, les, dns, comp)


def test_face_pullback_on_mixed_bc_grid(ins, oracle):
    les = mirror(ins, fx.setup_mixed(oracle), oracle)
    dns = ins.neuralclosure.dns_setup_of(les, 2)
    Φ = ins.FaceAverage()
    u, w = randf(ins, dns, 1), randf(ins, les, 2)
    Φu = Φ(u, les, 2, setup_dns=dns)
    ΦTw = Φ.pullback_(ins.vectorfield(dns), w, les, 2, dns)
    assert abs(dot(Φu, w) - dot(u, ΦTw)) <= TOL * nrm(Φu) * nrm(w)


@pytest.mark.parametrize("kind", ["FaceAverage", "VolumeAverage"])
def test_gradcheck_filters(ins, kind):
    import torch

    les, dns = periodic(ins, 4, 2), periodic(ins, 8, 2)
    u = randf(ins, dns, 9).requires_grad_(True)
    F = getattr(ins.ad, kind)
    assert torch.autograd.gradcheck(lambda x: F.apply(x, les, 2, dns), (u,), eps=1e-6, atol=1e-8)


# ------------------------------------------------------------------------------------ 5. error codes
def test_error_codes(ins, oracle):
    lib = ins._lib.load()
    les, dns = periodic(ins, 8, 2), periodic(ins, 16, 2)
    u, v = ins.vectorfield(dns), ins.vectorfield(les)
    up, vp, s = dns.ptr(u, True), les.ptr(v, True), les.stream
    INVALID, UNSUPPORTED = -1, -4
    assert lib.ins_filter_face_f64(les.handle, dns.handle, 2, up, vp, s) == 0
    for fn in (lib.ins_filter_face_f64, lib.ins_filter_volume_f64, lib.ins_filter_face_pullback_f64, lib.ins_filter_volume_pullback_f64):
        assert fn(None, dns.handle, 2, up, vp, s) == INVALID and fn(les.handle, None, 2, up, vp, s) == INVALID
        assert fn(les.handle, dns.handle, 3, up, vp, s) == INVALID  # comp · n_les != n_dns
        assert fn(les.handle, dns.handle, 0, up, vp, s) == INVALID
        assert fn(les.handle, dns.handle, 2, None, vp, s) == INVALID
    assert b"comp" in lib.ins_last_error() or b"null" in lib.ins_last_error()
    assert lib.ins_reconstruct_f64(None, les.handle, 2, vp, up, s) == INVALID
    assert lib.ins_reconstruct_f64(dns.handle, les.handle, 4, vp, up, s) == INVALID
    # same sizes, faces not nested
    x = np.linspace(0.0, 1.0, 17)
    x[4] += 0.4 / 16  # a fine face that should coincide with coarse face 2
    skew = ins.Setup(x=(x, np.linspace(0.0, 1.0, 17)), Re=1000.0)
    assert lib.ins_filter_face_f64(les.handle, skew.handle, 2, up, vp, s) == INVALID
    assert b"nested" in lib.ins_last_error()
    # wall-bounded grids: the face average works, the volume average and reconstruct say unsupported
    wl = mirror(ins, fx.setup2d(oracle), oracle)
    wd = ins.neuralclosure.dns_setup_of(wl, 2)
    wu, wv = ins.vectorfield(wd), ins.vectorfield(wl)
    assert lib.ins_filter_face_f64(wl.handle, wd.handle, 2, wd.ptr(wu, True), wl.ptr(wv, True), s) == 0
    assert lib.ins_filter_volume_f64(wl.handle, wd.handle, 2, wd.ptr(wu, True), wl.ptr(wv, True), s) == UNSUPPORTED
    assert lib.ins_filter_volume_pullback_f64(wl.handle, wd.handle, 2, wl.ptr(wv, True), wd.ptr(wu, True), s) == UNSUPPORTED
    assert lib.ins_reconstruct_f64(wd.handle, wl.handle, 2, wl.ptr(wv, True), wd.ptr(wu, True), s) == UNSUPPORTED
    with pytest.raises(ins.INSHipError):
        ins.VolumeAverage()(wu, wl, 2, setup_dns=wd)
    # a periodic coarse grid with a wall-bounded fine grid
    assert lib.ins_filter_face_f64(les.handle, wd.handle, 2, up, vp, s) == INVALID
