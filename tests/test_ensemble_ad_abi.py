"""The member-batched differentiable step, the part that needs no device: the C ABI of the operator-level ensemble entries (include/ins_hip.h against
`_lib.SIGNATURES`), the exports, and the refusals that are raised from host-side facts before a kernel is launched, each naming the per-trajectory route."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ins_amd as ins
from ins_amd import _lib
from ins_amd import neuralclosure as nc
from ins_amd.time_steppers import EnsembleCache
from tests.test_les_ensemble_abi import _prototypes

IN_PLACE = ["ins_rk_ensemble_t* ens", "double* {0}", "int64_t {1}", "void* stream"]
WANT = {
    "ins_rk_ensemble_momentum_f64": ["ins_rk_ensemble_t* ens", "double visc", "const double* U", "int64_t ustride", "double* F", "int64_t fstride", "void* stream"],
    "ins_rk_ensemble_project_f64": [a.format("U", "ustride") for a in IN_PLACE],
    "ins_rk_ensemble_apply_bc_u_pullback_f64": [a.format("G", "gstride") for a in IN_PLACE],
    "ins_rk_ensemble_momentum_pullback_f64": ["ins_rk_ensemble_t* ens", "double visc", "const double* U", "int64_t ustride", "const double* Phibar",
                                              "int64_t pstride", "double* Ubar", "int64_t bstride", "int accumulate", "void* stream"],
    "ins_rk_ensemble_project_pullback_f64": [a.format("G", "gstride") for a in IN_PLACE],
}
vp = C.c_void_p
BOUND = {
    "ins_rk_ensemble_momentum_f64": [vp, C.c_double, vp, C.c_int64, vp, C.c_int64, vp],
    "ins_rk_ensemble_project_f64": [vp, vp, C.c_int64, vp],
    "ins_rk_ensemble_apply_bc_u_pullback_f64": [vp, vp, C.c_int64, vp],
    "ins_rk_ensemble_momentum_pullback_f64": [vp, C.c_double, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, C.c_int, vp],
    "ins_rk_ensemble_project_pullback_f64": [vp, vp, C.c_int64, vp],
}


def test_header_declares_the_entries():
    protos = _prototypes()
    for name, params in WANT.items():
        assert protos.get(name) == params, (name, protos.get(name))


def test_lib_binds_the_entries():
    lib = _lib.load()
    for name, argtypes in BOUND.items():
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes), name
        assert getattr(lib, name).argtypes == argtypes


def test_exports():
    for f in ("ensemble_momentum_", "ensemble_project_", "ensemble_apply_bc_u_pullback_", "ensemble_momentum_pullback_", "ensemble_project_pullback_",
              "create_loss_post_ensemble", "wrappedclosure_ensemble"):
        assert callable(getattr(ins, f)), f
    for f in ("ensemble_apply_bc_u", "ensemble_momentum", "ensemble_project", "timestep_ensemble"):
        assert callable(getattr(ins.ad, f)) and f in ins.ad.__all__, f
    assert "create_loss_post_ensemble" in nc.__all__ and "wrappedclosure_ensemble" in nc.__all__


# ------------------------------------------------------------------------------------------------ host-side stand-ins: no Setup, no device
def _fake_setup(n=(32, 32), D=2, **kw):
    N = tuple(ni + 2 for ni in n)
    per = tuple((ins.PeriodicBC(), ins.PeriodicBC()) for _ in range(D))
    d = dict(grid=SimpleNamespace(N=N, dimension=D, Iu=tuple(tuple((1, ni - 1) for ni in N) for _ in range(D))), boundary_conditions=per, bodyforce=None,
             closure_model=None, temperature=None, device=torch.device("cpu"), Re=1000.0)
    d.update(kw)
    return SimpleNamespace(**d)


class psolver_spectral:  # `_ensemble_refusal` goes by the class name: no device behind this one
    pass


def _fake_cache(sp, B):
    c = EnsembleCache.__new__(EnsembleCache)
    c.setup, c.B = sp, B
    return c


def _fields(sp, B, dtype=torch.float64, pad=0):
    shape = sp.grid.N + (2,)
    m = int(np.prod(shape))
    flat = torch.zeros(B * (m + pad), dtype=dtype)
    return flat.as_strided((B,) + shape, (m + pad,) + tuple(int(np.prod(shape[:q])) for q in range(len(shape))))


@pytest.mark.parametrize("change, word", [
    (dict(setup=_fake_setup((16, 16, 16), D=3)), "3-D"),
    (dict(setup=_fake_setup(bodyforce=lambda *a: 0.0)), "body force"),
    (dict(setup=_fake_setup(temperature=object())), "temperature"),
    (dict(setup=_fake_setup((48, 32))), "48 x 32"),
    (dict(setup=_fake_setup((8, 32))), "8 x 32"),
    (dict(setup=_fake_setup(boundary_conditions=((ins.PeriodicBC(), ins.PeriodicBC()), (ins.DirichletBC(), ins.DirichletBC())))), "not periodic"),
    (dict(psolver=object.__new__(ins.f32.psolver_spectral32)), "Float32"),
    (dict(method=ins.RKMethods.FE11()), "one-stage"),
])
def test_create_loss_post_ensemble_refuses_on_host_facts(change, word):
    kw = dict(setup=_fake_setup(), method=ins.RKMethods.RK44(), psolver=psolver_spectral(), closure_model=None)
    kw.update(change)
    with pytest.raises(NotImplementedError) as e:
        ins.create_loss_post_ensemble(**kw)
    msg = str(e.value)
    assert word in msg and "ad.timestep per member, create_loss_post" in msg, msg


def test_mixed_step_sizes_are_refused_before_any_field_is_touched():
    loss = ins.create_loss_post_ensemble(setup=_fake_setup(), method=ins.RKMethods.RK44(), psolver=psolver_spectral(), closure_model=None)
    t = np.array([0.0, 1e-3, 2e-3])
    for other in (np.array([0.5, 0.5 + 1e-3, 0.5 + 3e-3]), np.array([0.0, 1e-3])):
        with pytest.raises(ValueError) as e:
            loss([dict(u=None, t=t), dict(u=None, t=other)], None)
        assert "create_loss_post" in str(e.value)
    # start times may differ: equal steps pass this check (the next thing the loss would do needs the device) ...
    assert np.allclose(nc._post_ensemble_steps([dict(t=t), dict(t=t + 0.25)]), 1e-3)
    assert np.allclose(nc._post_ensemble_steps([dict(t=1e-4 * np.arange(5)), dict(t=37.0 + 1e-4 * np.arange(5))]), 1e-4)
    # ... but only to the rounding of the saved times, 4 eps max|t|: a step one part in 1e10 longer is another step
    with pytest.raises(ValueError):
        nc._post_ensemble_steps([dict(t=t), dict(t=t * (1 + 1e-10))])


def test_wrappers_check_strides_dtype_and_member_count():
    sp = _fake_setup((16, 16))
    cache = _fake_cache(sp, 3)
    U = _fields(sp, 3)
    row_major = torch.zeros((3,) + sp.grid.N + (2,), dtype=torch.float64)
    for f in (ins.ensemble_project_, ins.ensemble_apply_bc_u_pullback_, ins.ensemble_project_pullback_):
        with pytest.raises(ValueError):
            f(cache, _fields(sp, 2))  # member count
        with pytest.raises(ValueError):
            f(cache, row_major)  # foreign strides
        with pytest.raises(TypeError):
            f(cache, _fields(sp, 3, torch.float32))
        with pytest.raises(TypeError):
            f(object(), U)
    with pytest.raises(ValueError) as e:
        ins.ensemble_momentum_(cache, U, U)  # F is U
    assert "in place" in str(e.value)
    with pytest.raises(ValueError):
        ins.ensemble_momentum_(cache, _fields(sp, 3), _fields(sp, 2))
    with pytest.raises(ValueError):
        ins.ensemble_momentum_pullback_(cache, U, U, _fields(sp, 3))
    # overlap of member ranges, not only equal base pointers: four members in one buffer, the output shifted by one member or by half a member
    W = _fields(sp, 4)
    with pytest.raises(ValueError):
        ins.ensemble_momentum_(cache, W[1:], W[:3])
    m = int(np.prod(sp.grid.N)) * 2
    buf = torch.zeros(5 * m, dtype=torch.float64)
    mk = lambda off: buf[off:off + 3 * m].as_strided(W[:3].shape, W[:3].stride())  # noqa: E731
    with pytest.raises(ValueError):
        ins.ensemble_momentum_pullback_(cache, mk(m // 2), mk(0), _fields(sp, 3))
    with pytest.raises(ValueError):
        ins.ensemble_momentum_pullback_(cache, mk(2 * m - 1), _fields(sp, 3), mk(0))
    with pytest.raises(ValueError):
        ins.ensemble_momentum_pullback_(cache, _fields(sp, 3), _fields(sp, 3), row_major)


def test_ad_entry_points_refuse_and_name_the_per_trajectory_route():
    sp = _fake_setup((16, 16))
    cache = _fake_cache(sp, 2)
    with pytest.raises(NotImplementedError) as e:
        ins.ad.timestep_ensemble(ins.RKMethods.RK44(), cache, _fields(sp, 2, torch.float32), 0.0, 1e-3)
    assert "Float32" in str(e.value) and "ad32.timestep" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        ins.ad.timestep_ensemble(ins.RKMethods.FE11(), cache, _fields(sp, 2), 0.0, 1e-3)
    assert "ad.timestep" in str(e.value)
    with pytest.raises(TypeError) as e:
        ins.ad.ensemble_momentum(object(), _fields(sp, 2))
    assert "ad.timestep" in str(e.value)
    with pytest.raises(ValueError):
        ins.ad.ensemble_project(cache, _fields(sp, 3))
    sp3 = _fake_setup((16, 16, 16), D=3)
    with pytest.raises(NotImplementedError) as e:
        ins.wrappedclosure_ensemble(lambda x, θ: x, sp3)
    assert "create_loss_post" in str(e.value)


@pytest.mark.parametrize("D, shape", [(2, (12, 10)), (3, (8, 6, 7))])
def test_batched_cnn_is_the_cnn_to_rounding(D, shape):
    """`cnn(..., batched=True)` lays the padded samples side by side and convolves once: the same sums per output value.  Off by default.  Bound: a
    convolution output is a dot product of K = 5·25 (2-D: 5 channels, 5 x 5) or fewer terms; another summation order changes it by at most K·eps·Σ|a||b|,
    over two layers and the gradient's further sums a few hundred eps: 1e-13 relative to the largest value."""
    sp = SimpleNamespace(grid=SimpleNamespace(dimension=D), device=torch.device("cpu"))
    kw = dict(setup=sp, radii=[2, 1], channels=[5, D], activations=[torch.tanh, None], use_bias=[True, False], rng=1)
    a, b = ins.cnn(**kw), ins.cnn(**kw, batched=True)
    assert a.batched is False and b.batched is True
    x = torch.randn(*shape, D, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    ya, yb = a(x), b(x)
    assert ya.shape == yb.shape == x.shape
    assert float((ya - yb).detach().abs().max()) <= 1e-13 * float(ya.detach().abs().max())
    ga = torch.autograd.grad((ya * ya).sum(), list(a.parameters()))
    gb = torch.autograd.grad((yb * yb).sum(), list(b.parameters()))
    for p, q in zip(ga, gb):
        assert float((p - q).abs().max()) <= 1e-13 * float(p.abs().max())
    # one sample: the same call
    assert float((a(x[..., :1]) - b(x[..., :1])).detach().abs().max()) <= 1e-13 * float(ya.detach().abs().max())
