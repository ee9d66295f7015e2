"""The numpy restatement of the DNS-to-LES filters (tests/filter_ref.py) has the properties the reference's filters have
(lib/NeuralClosure/test/filter.jl and the structure of the staggered grid): it is the yardstick of the GPU filter tests, pinned here."""
import numpy as np
import pytest

from tests import filter_ref as fr
from tests.fixtures import setup_periodic

EPS = np.finfo(np.float64).eps


def _inner(setup):
    return tuple(slice(1, n - 1) for n in setup.grid.N)


@pytest.mark.parametrize("D,n,n_les", [(2, 64, 32), (2, 64, 16), (3, 8, 4)])
def test_constant_field_is_preserved(oracle, D, n, n_les):
    comp = n // n_les
    les = setup_periodic(oracle, n_les, D)
    u = np.full((n + 2,) * D + (D,), 3.83, order="F")
    for v in (fr.face_average(u, les.grid.Iu, les.grid.N, comp), fr.volume_average(u, (n_les,) * D, comp)):
        for a in range(D):
            sl = tuple(slice(lo, hi) for lo, hi in les.grid.Iu[a])
            assert np.max(np.abs(v[sl + (a,)] - 3.83)) <= 4 * EPS * 3.83


@pytest.mark.parametrize("D,n_les,comp", [(2, 8, 4), (2, 6, 3), (3, 4, 2)])
def test_face_average_keeps_divergence_freeness(oracle, D, n_les, comp):
    o = oracle
    dns, les = setup_periodic(o, n_les * comp, D), setup_periodic(o, n_les, D)
    rng = np.random.default_rng(7)
    u = np.asfortranarray(rng.standard_normal(dns.grid.N + (D,)))
    u = o.apply_bc_u(u, 0.0, dns)
    u = o.apply_bc_u(o.project(u, dns, o.psolver_spectral(dns)), 0.0, dns)
    div_dns = np.max(np.abs(o.divergence(u, dns)[_inner(dns)]))
    v = o.apply_bc_u(fr.face_average(u, les.grid.Iu, les.grid.N, comp), 0.0, les)
    div_les = np.max(np.abs(o.divergence(v, les)[_inner(les)]))
    print(f"D={D} n_les={n_les} comp={comp}: max|div| DNS {div_dns:.3e}, face-averaged {div_les:.3e}")
    assert div_les <= 10 * div_dns


@pytest.mark.parametrize("D,n_les,comp", [(2, 8, 4), (2, 6, 3), (3, 4, 2), (2, 5, 1)])
def test_face_average_inverts_reconstruct(oracle, D, n_les, comp):
    les = setup_periodic(oracle, n_les, D)
    rng = np.random.default_rng(3)
    w = oracle.apply_bc_u(np.asfortranarray(rng.standard_normal(les.grid.N + (D,))), 0.0, les)
    back = fr.face_average(fr.reconstruct(w, (n_les,) * D, comp), les.grid.Iu, les.grid.N, comp)
    for a in range(D):
        sl = tuple(slice(lo, hi) for lo, hi in les.grid.Iu[a]) + (a,)
        assert np.max(np.abs(back[sl] - w[sl])) <= 4 * EPS * np.max(np.abs(w))


def _dense_transpose_apply(L, shape, w):
    """(dL)ᵀ w of a linear map L on numpy fields of `shape`, by unit probes (as tests/test_gpu_adjoint.py)."""
    n = int(np.prod(shape))
    out = np.empty(n)
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        out[k] = np.sum(w * L(e.reshape(shape, order="F")))
        e[k] = 0.0
    return out.reshape(shape, order="F")


@pytest.mark.parametrize("n_les,comp", [((3, 2, 2), 2), ((3, 2, 2), 3), ((4, 3), 4)])
@pytest.mark.parametrize("kind", ["face", "volume"])
def test_scatter_pullbacks_are_the_dense_transposes(oracle, kind, n_les, comp):
    """Every value of the scatter restatements against the transpose of the forward restatement.  A fine volume receives at most two coarse
    cotangents (the shared plane of an even volume average), each w / count against w · (1 / count): two roundings of terms ≤ max|w| each."""
    D = len(n_les)
    les = setup_periodic(oracle, n_les, D)
    shape_dns = tuple(comp * n + 2 for n in n_les) + (D,)
    rng = np.random.default_rng(17)
    w = np.asfortranarray(rng.standard_normal(tuple(les.grid.N) + (D,)))  # non-zero in the ghost volumes: the pullbacks must not read them
    if kind == "face":
        got = fr.face_average_pullback(w, les.grid.Iu, shape_dns[:-1], comp)
        ref = _dense_transpose_apply(lambda u: fr.face_average(u, les.grid.Iu, les.grid.N, comp), shape_dns, w)
    else:
        got = fr.volume_average_pullback(w, n_les, comp)
        ref = _dense_transpose_apply(lambda u: fr.volume_average(u, n_les, comp), shape_dns, w)
    assert got.shape == ref.shape and np.any(ref != 0)
    assert np.max(np.abs(got - ref)) <= 4 * EPS * np.max(np.abs(w))


def test_subdivide_is_nested():
    x = np.array([0.0, 0.1, 0.35, 1.0])
    for comp in (1, 2, 3):
        f = fr.subdivide(x, comp)
        assert len(f) == comp * 3 + 1 and np.array_equal(f[::comp], x) and np.all(np.diff(f) > 0)
