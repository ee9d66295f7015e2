"""CPU-side checks of the Float32 temperature pullback entry points (csrc/ins_temp_adjoint32.hip): declared in include/ins_hip.h as the float
twins of their `_f64` namesakes, bound in `_lib.py` with matching argument types, exported by the built library, and argument errors come back
as codes without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

NAMES = [
    "ins_apply_bc_temp_pullback_f32",
    "ins_gravity_adjoint_f32",
    "ins_convection_diffusion_temp_adjoint_f32",
    "ins_dissipation_adjoint_f32",
    "ins_temperature_pullback_f32",
]


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ins_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def _ctype(param):
    """The ctypes type `_lib.py` binds a C parameter declaration with."""
    t = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", param).strip()  # drop the parameter name
    if t == "const int32_t*":
        return C.POINTER(C.c_int32)
    if t.endswith("*"):
        return C.c_void_p
    return {"int": C.c_int, "float": C.c_float, "double": C.c_double}[t]


def test_declared_as_float_twins_of_the_f64_entries():
    protos = _prototypes()
    for n in NAMES:
        assert n in protos, f"{n} is not declared in ins_hip.h"
        twin = protos[n[:-4] + "_f64"]
        # the same argument order and names; every double becomes a float, the descriptor stays ins_temperature_desc_t
        assert protos[n] == [a.replace("double", "float") for a in twin], (n, protos[n], twin)
    assert "const ins_temperature_desc_t* desc" in protos["ins_temperature_pullback_f32"]


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    protos = _prototypes()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [_ctype(p) for p in protos[n]], (n, args, protos[n])
    for f in ("apply_bc_temp_pullback32_", "gravity_adjoint32_", "convection_diffusion_temp_adjoint32_", "dissipation_adjoint32_",
              "temperature_pullback32_"):
        assert callable(getattr(ins_amd.f32, f))
    for f in ("apply_bc_temp", "gravity", "convection_diffusion_temp", "dissipation"):  # module attributes, not in __all__
        assert callable(getattr(ins_amd.ad32, f)) and f not in ins_amd.ad32.__all__


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    calls = [
        lambda: lib.ins_apply_bc_temp_pullback_f32(None, None, None, None),
        lambda: lib.ins_gravity_adjoint_f32(None, 0, 0.0, None, None, None),
        lambda: lib.ins_convection_diffusion_temp_adjoint_f32(None, 0.0, None, None, None, None, None, None),
        lambda: lib.ins_dissipation_adjoint_f32(None, 0.0, 0.0, None, None, None, None),
        lambda: lib.ins_temperature_pullback_f32(None, None, 0.0, None, None, None, None, None, None, None),
    ]
    for call in calls:
        assert call() == -1
        assert b"null" in lib.ins_last_error()
