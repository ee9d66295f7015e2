"""CPU-side checks of the Float32 DNS-to-LES filters (csrc/ins_filter32.hip) and of the Float32 glue of `ins_amd.neuralclosure`: the six new
entries are declared, bound and exported, argument errors come back as codes without a device, mixed precisions are a TypeError before anything is
launched, and the training arrays, the CNN and the data loaders keep float32 (float64 stays the default everywhere)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

FILTER = ["const ins_grid_t* les", "const ins_grid_t* dns", "int comp", "const float* {a}", "float* {b}", "void* stream"]
PROTOS = {
    "ins_filter_face_f32": [p.format(a="u", b="v") for p in FILTER],
    "ins_filter_volume_f32": [p.format(a="u", b="v") for p in FILTER],
    "ins_reconstruct_f32": ["const ins_grid_t* dns", "const ins_grid_t* les", "int comp", "const float* v", "float* u", "void* stream"],
    "ins_filter_face_pullback_f32": [p.format(a="w", b="ubar") for p in FILTER],
    "ins_filter_volume_pullback_f32": [p.format(a="w", b="ubar") for p in FILTER],
    "ins_apply_bc_u_dudt_f32": ["const ins_grid_t* grid", "float* u", "void* stream"],
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ins_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def test_declared_exported_and_bound():
    import ins_amd

    lib, protos = ins_amd._lib.load(), _prototypes()
    for n, want in PROTOS.items():
        assert protos.get(n) == want, (n, protos.get(n))
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [C.c_int if p.startswith("int ") else C.c_void_p for p in want], (n, args)
    # the float filters are the twins of the fp64 ones: the same argument order and names
    for n in list(PROTOS)[:5]:
        assert [a.replace("double", "float") for a in protos[n.replace("_f32", "_f64")]] == protos[n]


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    for n in list(PROTOS)[:5]:
        assert getattr(lib, n)(None, None, 2, None, None, None) == -1, n
        assert b"null" in lib.ins_last_error()
    assert lib.ins_apply_bc_u_dudt_f32(None, None, None) == -1
    assert b"null" in lib.ins_last_error()


def test_filters_refuse_mixed_precisions_before_any_launch():
    """`u` and `v` of different precisions: a TypeError that names both dtypes, raised before a setup is touched (setup_les=None: no device)."""
    import ins_amd as ins

    u32, v64 = torch.zeros(6, 6, 2, dtype=torch.float32), torch.zeros(4, 4, 2, dtype=torch.float64)
    u64, v32 = u32.double(), v64.float()
    for Φ in (ins.FaceAverage(), ins.VolumeAverage()):
        for v, u in ((v64, u32), (v32, u64)):
            with pytest.raises(TypeError, match="float32.*float64|float64.*float32"):
                Φ(v, u, None, 2)
            with pytest.raises(TypeError, match="float32.*float64|float64.*float32"):
                Φ.pullback_(u, v, None, 2)
    with pytest.raises(TypeError, match="float32.*float64|float64.*float32"):
        ins.reconstruct_(u32, v64, None, None, 2)


def test_filtersaver_refuses_mixed_precisions_in_initialize():
    """A float32 state with an fp64 solver (and the reverse) is a TypeError in `initialize`, before scratch is allocated or a kernel launched
    (the setups are None here: no device)."""
    import ins_amd as ins

    f32 = ins.f32
    ps32, ps64 = object.__new__(f32.psolver_spectral32), object.__new__(ins.psolver_spectral)  # only their class is looked at
    wrap32 = object.__new__(f32.psolver_wrap32)
    s32 = dict(u=torch.zeros(6, 6, 2, dtype=torch.float32), temp=None, t=0.0, n=0)
    s64 = dict(u=torch.zeros(6, 6, 2, dtype=torch.float64), temp=None, t=0.0, n=0)
    for state, dns_ps, les_ps in ((s32, ps64, ps32), (s32, ps32, ps64), (s32, ps64, ps64), (s64, ps32, ps64), (s64, ps64, wrap32)):
        saver = ins.filtersaver(None, [None], [ins.FaceAverage()], [2], dns_ps, [les_ps], nupdate=1)
        with pytest.raises(TypeError, match="float32"):
            saver.initialize(lambda: state)


def test_create_io_arrays_keeps_the_dtype_of_the_data():
    import ins_amd as ins

    class G:
        dimension, N = 2, (6, 6)
        Iu = (((1, 5), (1, 5)), ((1, 5), (1, 5)))

    class S:
        grid = G

    rng = np.random.default_rng(0)
    for dt in (np.float32, np.float64):
        traj = dict(u=rng.standard_normal((6, 6, 2, 3)).astype(dt), c=rng.standard_normal((6, 6, 2, 3)).astype(dt), t=np.arange(3.0))
        io = ins.create_io_arrays([traj, traj], S)
        for k in ("u", "c"):
            assert io[k].dtype == dt and io[k].shape == (4, 4, 2, 6)
            assert np.array_equal(io[k][..., :3], traj[k][1:5, 1:5])


def test_cnn_dtype():
    import ins_amd as ins

    class G:
        dimension = 2

    class S:
        grid, device = G, torch.device("cpu")

    kw = dict(setup=S, radii=[1, 1], channels=[4, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=0)
    m32, m64 = ins.cnn(**kw, dtype=torch.float32), ins.cnn(**kw)
    assert all(p.dtype == torch.float32 for p in m32.parameters())
    assert all(p.dtype == torch.float64 for p in m64.parameters())
    x = torch.randn(8, 8, 2, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    with torch.no_grad():
        y, y64 = m32(x, None), m64(x.double(), None)
    assert y.dtype == torch.float32 and y.shape == x.shape and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert y64.dtype == torch.float64 and y64.shape == x.shape
    with pytest.raises(TypeError):
        ins.cnn(**kw, dtype=torch.float16)


def test_dataloaders_dtype():
    import ins_amd as ins

    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((4, 4, 2, 7)).astype(np.float32), rng.standard_normal((4, 4, 2, 7)).astype(np.float32)
    for dtype, want in ((torch.float32, torch.float32), (None, torch.float64)):
        (bx, by), _ = ins.create_dataloader_prior((x, y), batchsize=3, device="cpu", dtype=dtype)(np.random.default_rng(1))
        assert bx.dtype == want and by.dtype == want and bx.shape == (4, 4, 2, 3)
        traj = [dict(u=rng.standard_normal((6, 6, 2, 5)).astype(np.float32), t=np.arange(5.0))]
        data, _ = ins.create_dataloader_post(traj, ntrajectory=1, nunroll=2, device="cpu", dtype=dtype)(np.random.default_rng(1))
        assert data[0]["u"].dtype == want and data[0]["u"].shape == (6, 6, 2, 3) and data[0]["t"].dtype == np.float64
