"""Ensemble filtered-DNS data, the part that needs no device: the C ABI of the member-batched right-hand side and filters (include/ins_hip.h against
`_lib.SIGNATURES`), the exports, and the refusals of `create_les_data_ensemble` and `Φ.members`, which are raised from host-side facts before a setup
exists or a kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ins_amd as ins
from ins_amd import _lib
from ins_amd import neuralclosure as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

MEMBERS_SIG = ["const ins_grid_t* les", "const ins_grid_t* dns", "int comp", "int nbatch", "const double* u", "int64_t ustride", "double* v", "int64_t vstride",
               "void* stream"]
WANT = {
    "ins_rk_ensemble_rhs_f64": ["ins_rk_ensemble_t* ens", "double visc", "const double* U", "int64_t ustride", "double* F", "int64_t fstride", "void* stream"],
    "ins_filter_face_members_f64": MEMBERS_SIG,
    "ins_filter_volume_members_f64": MEMBERS_SIG,
}
vp = C.c_void_p
BOUND = {
    "ins_rk_ensemble_rhs_f64": [vp, C.c_double, vp, C.c_int64, vp, C.c_int64, vp],
    "ins_filter_face_members_f64": [vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int64, vp],
    "ins_filter_volume_members_f64": [vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int64, vp],
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ins_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
    return out


def test_header_declares_the_three_entries():
    protos = _prototypes()
    for name, params in WANT.items():
        assert protos.get(name) == params, (name, protos.get(name))


def test_lib_binds_the_three_entries():
    for name, argtypes in BOUND.items():
        assert _lib.SIGNATURES[name] == (C.c_int, argtypes), name
    lib = _lib.load()
    for name in BOUND:
        assert getattr(lib, name).argtypes == BOUND[name]


def test_exports():
    assert "create_les_data_ensemble" in nc.__all__
    assert ins.create_les_data_ensemble is nc.create_les_data_ensemble
    assert callable(ins.ensemble_rhs_) and callable(ins.ensemble_apply_bc_u_)
    for Φ in (ins.FaceAverage(), ins.VolumeAverage()):
        assert callable(Φ.members)
    assert nc.AbstractFilter.members is not None


OK = dict(ntrajectory=2, D=2, Re=1000.0, lims=(0.0, 1.0), nles=(16, 32), ndns=64, filters=(ins.FaceAverage(),), tburn=0.0, tsim=0.01, savefreq=2, Δt=1e-3)


@pytest.mark.parametrize("change, word", [
    (dict(Δt=None), "Δt=None"),
    (dict(D=3), "D = 3"),
    (dict(ndns=96, nles=(48,)), "ndns = 96"),
    (dict(ndns=2048, nles=(32,)), "ndns = 2048"),
    (dict(nles=(8,)), "nles = 8"),
    (dict(nles=(16, 24)), "nles = 24"),
    (dict(dtype=torch.float32), "float32"),
    (dict(processors=dict(log=object())), "processors"),
    (dict(bodyforce=lambda *a: 0.0), "bodyforce"),
    (dict(closure_model=lambda u, θ: u), "closure_model"),
    (dict(boundary_conditions=None), "boundary_conditions"),
])
def test_create_les_data_ensemble_refuses_before_any_setup(change, word, monkeypatch):
    def no_setup(*a, **k):
        raise AssertionError("a Setup was created before the refusal")

    monkeypatch.setattr(nc, "Setup", no_setup)
    with pytest.raises(NotImplementedError) as e:
        ins.create_les_data_ensemble(**{**OK, **change})
    msg = str(e.value)
    assert word in msg and "create_les_data once per seed" in msg, msg


def test_members_refuses_float32_by_type_alone():
    v32 = torch.zeros(2, 4, 4, 2, dtype=torch.float32)
    for Φ in (ins.FaceAverage(), ins.VolumeAverage()):
        with pytest.raises(TypeError) as e:
            Φ.members(v32, v32, None, 2)  # the precision is checked before the setups are touched
        assert "V[b], U[b], setup_les, comp" in str(e.value) and type(Φ).__name__ in str(e.value)


def test_host_side_shape_checks_of_the_member_stride():
    from types import SimpleNamespace

    from ins_amd.time_steppers import _member_stride

    sp = SimpleNamespace(grid=SimpleNamespace(N=(6, 5), dimension=2), device=torch.device("cpu"))
    U = torch.zeros(3, 2, 5, 6, dtype=torch.float64).permute(0, 3, 2, 1)
    assert _member_stride(sp, U) == 60 and _member_stride(sp, U[:1]) == 60
    assert _member_stride(sp, torch.zeros(3, 100, dtype=torch.float64).as_strided((3, 6, 5, 2), (100, 1, 6, 30))) == 100  # padding between members
    with pytest.raises(ValueError):
        _member_stride(sp, U, 4)
    with pytest.raises(ValueError):
        _member_stride(sp, torch.zeros(3, 6, 5, 2, dtype=torch.float64))  # row-major members
    with pytest.raises(TypeError):
        _member_stride(sp, np.zeros((3, 6, 5, 2)))
