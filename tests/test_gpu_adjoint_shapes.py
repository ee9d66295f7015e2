"""GPU: the pullback kernels (csrc/ins_adjoint.hip, csrc/ins_adjoint_kernels.h and their Float32 twins) at the shapes where an index map can go wrong.

  A1. the tiled momentum pullback on all-periodic uniform boxes with three different sizes and three different spacings (on a cube the metric
      constants, the sizes and the strides of the three directions can be swapped without changing a number), at the edges of its 62-column x tiles,
      4-row workgroups in 8 bands and 32-plane z chunks: value by value against the CPU oracle at probes, and every value against the generic kernel;
  A2. the cotangent-combining instantiation (INS_ADJ_STAGE_FUSED=1) and the native reverse step on such a box, against the unrolled autograd path
      with the tiled kernel switched off;
  A3. the generic gather pullbacks across the seams of their 64 x 4 tiles on wall-bounded stretched grids (tests/test_gpu_stencil_tiles.make_setup):
      every identity of tests/test_gpu_adjoint.py, tests/test_gpu_temp_adjoint.py and tests/test_gpu_tensorclosure.py through their helpers, and
      columns of the oracle's transposes at probes on the boundaries and the seams (a scalar identity cannot place an error);
  A4. the Float32 twins on the same grids, through the helpers and bounds of tests/test_gpu_adjoint32.py and tests/test_gpu_temp_adjoint32.py.

Every tolerance is imported from the file whose check is repeated.  The oracle columns are exact: the operators are linear or quadratic, so a unit
probe (a central difference with step 1 for the quadratic ones) gives the Jacobian column without truncation, as tests/test_gpu_adjoint.py item 3.
"""
import itertools

import numpy as np
import pytest

from tests import fixtures as fx
from tests import test_gpu_adjoint32 as a32
from tests import test_gpu_temp_adjoint32 as t32
from tests.test_gpu_ad_timesteps import grad_rollout, grad_unrolled, rel
from tests.test_gpu_adjoint import TOL, _u0, check_convection_and_momentum_pullbacks, check_linear_transposes, mirror, oracle_transpose_cases, rand
from tests.test_gpu_fields import with_temperature
from tests.test_gpu_stencil_tiles import make_setup
from tests.test_gpu_temp_adjoint import check_fused_pullback, check_transpose_identities
from tests.test_gpu_tensorclosure import check_divoftensor_transpose

pytestmark = pytest.mark.gpu

LENGTHS = (1.0, 0.7, 1.9)


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


# ------------------------------------------------------------------------------------ probes
def choose(axes, cap, seed):
    """Points of the product of `axes` (lists of values): all of them if there are at most `cap`, else a fixed sample of `cap` that holds every value of
    every axis at least once."""
    full = list(itertools.product(*axes))
    if len(full) <= cap:
        return full
    cover = [tuple(ax[i % len(ax)] for ax in axes) for i in range(max(len(ax) for ax in axes))]
    rest = sorted(set(full) - set(cover))
    rng = np.random.default_rng(seed)
    picked = cover + [rest[i] for i in rng.choice(len(rest), cap - len(cover), replace=False)]
    for d, ax in enumerate(axes):
        assert {p[d] for p in picked} == set(ax)
    return picked


def inbox(values, n):
    return sorted({v for v in values if 0 <= v < n})


def columns(L, shape, cot, probes):
    """((dL)^T cot)[k] = <cot, L(e_k)> for the indices k of `probes`, L linear on numpy fields of `shape`."""
    out = np.empty(len(probes))
    e = np.zeros(shape, order="F")
    for m, k in enumerate(probes):
        e[k] = 1.0
        out[m] = np.sum(cot * L(e))
        e[k] = 0.0
    return out


def at(field, probes):
    return np.array([field[k] for k in probes])


def probe_err(got, ref):
    """relmax of tests/test_gpu_adjoint.py over the probes"""
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


# ------------------------------------------------------------------------------------ A1. the tiled momentum pullback against the oracle
# padded sizes N = n + 2
BOXES = {
    "a_62x5x33": (62, 5, 33),    # exactly one full x tile; 2 row-tiles, so 6 empty bands; a z chunk of one plane
    "b_63x37x4": (63, 37, 4),    # a second x tile with one output column; 10 row-tiles, so a band cut short; N2 below one chunk
    "c_125x9x32": (125, 9, 32),  # a third tile with one column; a chunk that ends on the last plane
    "d_10x34x6": (10, 34, 6),    # one partial tile; 9 row-tiles
}


def aniso_box(ins, o, N):
    """(oracle setup, library setup) of the all-periodic uniform box with padded sizes N and side lengths LENGTHS."""
    n = tuple(Ni - 2 for Ni in N)
    x = tuple(np.linspace(0.0, L, ni + 1) for L, ni in zip(LENGTHS, n))
    so, sp = o.make_setup(x, Re=1000.0), ins.Setup(x=x, Re=1000.0)
    assert tuple(so.grid.N) == tuple(N) and tuple(sp.grid.N) == tuple(N)
    h = [L / ni for L, ni in zip(LENGTHS, n)]
    for a, b in itertools.combinations(h, 2):
        assert abs(a - b) > 0.1 * max(a, b), "two spacings within 10 % of each other"
    assert ins._lib.load().ins_grid_is_uniform_exact(sp.handle), "the tiled pullback serves this box"
    return so, sp


@pytest.mark.parametrize("box", list(BOXES))
def test_tiled_momentum_pullback_matches_oracle_on_anisotropic_boxes(ins, oracle, box):
    import torch

    o, N = oracle, BOXES[box]
    so, sp = aniso_box(ins, o, N)
    shape = tuple(N) + (3,)
    u, w, base = fx.randn_field(shape, 70), fx.randn_field(shape, 71), fx.randn_field(shape, 72)  # non-zero in the ghost volumes
    ug, wg, bg = (ins.from_numpy(sp, x) for x in (u, w, base))
    res = {}
    for off in (0, 1):
        with ins._lib.options(INS_DISABLE_ADJ_TILED=off):
            res[off] = ins.momentum_pullback_(ins.vectorfield(sp), wg, ug, sp)
            res[off, "acc"] = ins.momentum_pullback_(ins.copyfield(bg), wg, ug, sp, accumulate=True)
    # tiled against generic, every value (tests/test_gpu_adjoint.py item 5)
    gen = float((res[0] - res[1]).abs().max()) / float(res[1].abs().max())
    gen_acc = float((res[0, "acc"] - res[1, "acc"]).abs().max()) / float(res[1, "acc"].abs().max())
    # against the oracle at probes: (J^T w)[k] = <w, (M(u + e_k) - M(u - e_k)) / 2>, exact because M is quadratic
    axes = [inbox([0, 1, 2, 60, 61, 62, 63, N[0] - 2, N[0] - 1], N[0]), inbox([0, 1, 3, 4, 5, N[1] - 2, N[1] - 1], N[1]),
            inbox([0, 1, 30, 31, 32, N[2] - 2, N[2] - 1], N[2]), [0, 1, 2]]
    probes = choose(axes, 100, seed=73)
    ref = columns(lambda x: (o.momentum(u + x, None, 0.0, so) - o.momentum(u - x, None, 0.0, so)) / 2, shape, w, probes)
    err = probe_err(at(ins.to_numpy(res[0]), probes), ref)
    err_acc = float(np.max(np.abs(at(ins.to_numpy(res[0, "acc"]), probes) - (at(base, probes) + ref))) / np.max(np.abs(ref)))
    print(f"tiled momentum pullback, box {box}: vs oracle at {len(probes)} probes {err:.3e}, accumulate {err_acc:.3e}; vs generic {gen:.3e}, accumulate {gen_acc:.3e}")
    # the route: no counter exposes it, so the switch must change at least one bit
    assert not torch.equal(res[0], res[1]), "INS_DISABLE_ADJ_TILED changes nothing: the tiled kernel did not run"
    assert gen <= TOL and gen_acc <= TOL, (gen, gen_acc)
    assert np.max(np.abs(ref)) > 0
    assert err <= TOL, err
    assert err_acc <= TOL, err_acc


# ------------------------------------------------------------------------------------ A2. PhiComb and the native reverse step on a non-cube
def test_reverse_step_routes_agree_on_an_anisotropic_box(ins, oracle):
    """N = 66 x 8 x 42: a ragged second x tile, 2 row-tiles, z chunks of 32 + 10.  RK44, two steps, a checkpoint at every step.  The unrolled autograd
    path with INS_DISABLE_ADJ_TILED=1 touches no tiled kernel and is the reference."""
    import torch

    _, sp = aniso_box(ins, oracle, (66, 8, 42))
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    u0, w = _u0(ins, sp, ps, 80), rand(ins, sp, True, 81)
    g = {"ad.timesteps": grad_rollout(ins, method, sp, ps, u0, w, 2, 1)}
    with ins._lib.options(INS_ADJ_STAGE_FUSED=1):
        g["ad.timesteps, fused reverse stage"] = grad_rollout(ins, method, sp, ps, u0, w, 2, 1)
    g["unrolled ad.timestep"] = grad_unrolled(ins, method, sp, ps, u0, w, 2)
    with ins._lib.options(INS_DISABLE_ADJ_TILED=1):
        ref = grad_unrolled(ins, method, sp, ps, u0, w, 2)
    assert not torch.equal(g["unrolled ad.timestep"], ref), "INS_DISABLE_ADJ_TILED changes nothing: the tiled kernel did not run"
    r = {k: rel(v, ref) for k, v in g.items()}
    print("reverse step on 66 x 8 x 42 against the generic unrolled path:", ", ".join(f"{k}: {v:.3e}" for k, v in r.items()))
    for k, v in r.items():
        assert v <= TOL, (k, v)


# ------------------------------------------------------------------------------------ A3. generic pullbacks across tile seams
# (D, padded N0, padded N1, kind) of tests/test_gpu_stencil_tiles.make_setup: "mixed" is Dirichlet / Pressure in x, Symmetric in y, periodic in z on a
# tanh x cosine grid; N0 = 65 and 130 put the pressure side into a ragged x tile, N1 = 34 and 37 the upper wall into a second row-band.  No tiled 2-D
# pullback exists, so the periodic 130 x 37 runs the generic kernels on a periodic grid.
GRIDS = {"mixed3d": (3, 65, 34, "mixed"), "mixed2d": (2, 130, 37, "mixed"), "periodic2d": (2, 130, 37, "periodic")}
MIXED = ["mixed3d", "mixed2d"]


def grid(o, name):
    D, N0, N1, kind = GRIDS[name]
    so = make_setup(o, D, N0, N1, kind)
    assert tuple(so.grid.N)[:2] == (N0, N1)
    return so


@pytest.mark.parametrize("name", list(GRIDS))
def test_transpose_identities_across_tile_seams(ins, oracle, name):
    sp = mirror(ins, grid(oracle, name), oracle)
    check_linear_transposes(ins, sp, [ins.psolver_direct(sp)])
    check_convection_and_momentum_pullbacks(ins, sp)
    check_divoftensor_transpose(ins, sp)


@pytest.mark.parametrize("name", list(GRIDS))
def test_temperature_pullbacks_across_tile_seams(ins, oracle, name):
    check_transpose_identities(ins, with_temperature(ins, oracle, grid(oracle, name), "any", gdir=1))
    for diss in (True, False):
        check_fused_pullback(ins, with_temperature(ins, oracle, grid(oracle, name), "any", gdir=1, dodissipation=diss))


ORACLE_OPS = ["convection", "diffusion", "pressuregradient", "apply_bc_u", "apply_bc_p"]


@pytest.mark.parametrize("name", list(GRIDS))
def test_pullback_columns_match_oracle_across_tile_seams(ins, oracle, name):
    o = oracle
    so = grid(o, name)
    sp = mirror(ins, so, o)
    N, D = tuple(so.grid.N), so.grid.D
    # the first two and last two indices of each direction, the x seams of the 64-wide tiles, the y seams of the 4-row tiles and of the row-bands
    axes = [inbox([0, 1, N[0] - 2, N[0] - 1, 63, 64, 65, 127, 128], N[0]), inbox([0, 1, N[1] - 2, N[1] - 1, 3, 4, 31, 32, 33], N[1])]
    if D == 3:
        axes.append(inbox([0, 1, N[2] - 2, N[2] - 1], N[2]))
    cases = {c[0]: c for c in oracle_transpose_cases(ins, o, so, sp)}
    for seed, what in enumerate(ORACLE_OPS):
        _, L, shape, cot, got = cases[what]
        probes = choose(axes + ([list(range(D))] if len(shape) > D else []), 60, seed=90 + seed)
        ref = columns(L, shape, cot, probes)
        err = probe_err(at(ins.to_numpy(got), probes), ref)
        print(f"{name} {what}, {len(probes)} probes: {err:.3e}")
        assert np.max(np.abs(ref)) > 0 and err <= TOL, (what, err)


# ------------------------------------------------------------------------------------ A4. Float32
@pytest.mark.parametrize("name", MIXED)
def test_float32_pullbacks_across_tile_seams(ins, oracle, name):
    sp = mirror(ins, grid(oracle, name), oracle)
    a32.check_transpose_identities(ins, sp, name)
    a32.check_values_against_fp64(ins, sp, name)


@pytest.mark.parametrize("name", MIXED)
def test_float32_temperature_pullbacks_across_tile_seams(ins, oracle, name):
    sp = with_temperature(ins, oracle, grid(oracle, name), "any", gdir=1)
    t32.check_transpose_identities(ins, sp, f"{name}/any/gdir1")
    t32.check_values_against_fp64(ins, sp, f"{name}/any/gdir1")
