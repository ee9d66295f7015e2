"""GPU: the index maps of the generic stencil kernels (csrc/ins_stencil.h), at the smallest shapes where they can go wrong.

Padded N0 in {64, 65, 130}: exactly one x-tile of 64, one volume into a second tile, a third ragged tile.  Padded N1 in {5, 34, 37}: 2, 9
and 10 row-tiles of 4, i.e. nty_l = 1, 2, 2 rows of tiles per XCD band, so the banded map has empty bands, a band cut short in the middle
and a full set.  3-D adds padded N2 = 4.  One mixed non-periodic stretched grid and one all-periodic uniform grid per shape.

  forward  (CPU oracle, the parity tolerance OP_TOL of tests/test_gpu_parity.py and tests/test_gpu_fields.py):
           plain grid: momentum, divergence;  banded grid: vorticity, interpolate_u_p;  boundary lines: apply_bc_u then apply_bc_p
  adjoint  (transpose identity, the tolerance of tests/test_gpu_adjoint.py and tests/test_gpu_temp_adjoint.py, random fields that are
           non-zero in the ghost volumes): plain grid: divergence_adjoint;  banded grid: gravity_adjoint
"""
import numpy as np
import pytest

from tests import fixtures as fx
from tests.test_gpu_adjoint import check_transpose, rand
from tests.test_gpu_fields import OP_TOL, relmax, with_temperature

pytestmark = pytest.mark.gpu

N0S, N1S, N2 = (64, 65, 130), (5, 34, 37), 4


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def make_setup(o, D, N0, N1, kind):
    """Oracle setup with padded sizes (N0, N1[, N2]): every BC used here has one ghost volume per side except a LEFT PressureBC."""
    n = (N0 - 2, N1 - 2, N2 - 2)[:D]
    if kind == "periodic":
        return fx.setup_periodic(o, n, D=D)
    x = (o.tanh_grid(0.0, 5.0, n[0], 1.2), o.cosine_grid(0.0, 1.0, n[1]), np.linspace(0.0, 0.8, n[2] + 1) if D == 3 else None)[:D]
    bcs = ((o.DirichletBC(), o.PressureBC()), (o.SymmetricBC(), o.SymmetricBC()), (o.PeriodicBC(), o.PeriodicBC()))[:D]
    return o.make_setup(x, bcs, Re=1000.0)


@pytest.mark.parametrize("kind", ["mixed", "periodic"])
@pytest.mark.parametrize("N1", N1S)
@pytest.mark.parametrize("N0", N0S)
@pytest.mark.parametrize("D", [2, 3])
def test_index_maps(ins, oracle, D, N0, N1, kind):
    o = oracle
    so = make_setup(o, D, N0, N1, kind)
    sp = with_temperature(ins, o, so, "any", gdir=1)
    g = so.grid
    assert tuple(g.N) == (N0, N1, N2)[:D]

    # forward, against the oracle
    raw_u, raw_p = fx.randn_field(g.N + (D,), 4), fx.randn_field(g.N, 5)
    u_h = o.apply_bc_u(raw_u, 0.0, so)
    assert np.array_equal(ins.to_numpy(ins.apply_bc_u_(ins.from_numpy(sp, raw_u), 0.0, sp)), u_h)
    assert np.array_equal(ins.to_numpy(ins.apply_bc_p_(ins.from_numpy(sp, raw_p), 0.0, sp)), o.apply_bc_p(raw_p, 0.0, so))
    u = ins.from_numpy(sp, u_h)
    F0 = fx.randn_field(g.N + (D,), 3)  # momentum! overwrites F: start from garbage
    assert relmax(ins.to_numpy(ins.momentum_(ins.from_numpy(sp, F0), u, None, 0.0, sp)), o.momentum(u_h, None, 0.0, so)) < OP_TOL
    assert relmax(ins.to_numpy(ins.divergence(u, sp)), o.divergence(u_h, so)) < OP_TOL
    assert relmax(ins.to_numpy(ins.vorticity(u, sp)), o.vorticity(u_h, so)) < OP_TOL
    assert relmax(ins.to_numpy(ins.interpolate_u_p(u, sp)), o.interpolate_u_p(u_h, so)) < OP_TOL

    # adjoint, by the transpose identity on the whole padded arrays
    v, w = rand(ins, sp, True, 1), rand(ins, sp, True, 2)
    p, q = rand(ins, sp, False, 3), rand(ins, sp, False, 4)
    check_transpose(ins.divergence(v, sp), v, q, ins.divergence_adjoint_(ins.vectorfield(sp), q, sp))
    check_transpose(ins.gravity(p, sp), p, w, ins.gravity_adjoint_(ins.scalarfield(sp), w, sp))
