"""CPU-side checks of the Float32 tensor-closure entry points (csrc/ins_tensorclosure32.hip): exported, bound with the argument lists of
their `_f64` twins, argument errors come back as codes without a device, and the Python layers above them exist."""
import ctypes as C

NAMES = [
    "ins_tensorinvariants_f32",
    "ins_tensorclosure_stress_f32",
    "ins_tensorclosure_pullback_f32",
    "ins_divoftensor_f32",
    "ins_divoftensor_adjoint_f32",
]


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert (res, args) == ins_amd._lib.SIGNATURES[n.replace("_f32", "_f64")], f"{n} differs from its _f64 twin"
    for f in ("tensorfield32", "tensorinvariants32_", "tensorclosure_stress32_", "tensorclosure_pullback32_", "divoftensor32_",
              "divoftensor_adjoint32_"):
        assert callable(getattr(ins_amd.f32, f)), f
    for f in ("apply_bc_p", "apply_bc_p_fields", "tensorinvariants", "tensorclosure_stress", "divoftensor", "lastdimcontract",
              "smagorinsky_closure"):
        assert callable(getattr(ins_amd.ad32, f)), f
    assert ins_amd.ad32.__all__ == ["apply_bc_u", "momentum", "project", "timestep"]


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    calls = [
        lambda: lib.ins_tensorinvariants_f32(None, None, None, None),
        lambda: lib.ins_tensorclosure_stress_f32(None, None, None, None, None),
        lambda: lib.ins_tensorclosure_pullback_f32(None, None, None, None, None, None, None, 0, None),
        lambda: lib.ins_divoftensor_f32(None, None, None, None),
        lambda: lib.ins_divoftensor_adjoint_f32(None, None, None, None),
    ]
    for call in calls:
        assert call() == -1
        assert b"null" in lib.ins_last_error()


def test_tensorclosure_dtype_argument():
    import inspect

    import torch

    import ins_amd

    p = inspect.signature(ins_amd.neuralclosure.tensorclosure).parameters
    assert p["dtype"].default is torch.float64
