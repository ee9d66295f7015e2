"""CPU-side checks of the Float32 Smagorinsky closure and steady body force entry points (csrc/ins_smagforce32.hip, csrc/ins_f32.hip): declared in
include/ins_hip.h as the float twins of their fp64 namesakes, bound in `_lib.py` with matching argument types, exported by the built library, and
argument errors come back as codes without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

# new entry -> its fp64 twin
TWINS = {
    "ins_smagtensor_f32": "ins_smagtensor_f64",
    "ins_smagorinsky_force_f32": "ins_smagorinsky_force_f64",
    "ins_rk_set_closure_f32": "ins_rk_set_closure",
    "ins_rk_set_bodyforce_f32": "ins_rk_set_bodyforce",
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ins_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def _ctype(param):
    """The ctypes type `_lib.py` binds a C parameter declaration with."""
    t = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", param).strip()  # drop the parameter name
    if t.endswith("*"):
        return C.c_void_p
    return {"int": C.c_int, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}[t]


def test_declared_as_float_twins_of_the_f64_entries():
    protos = _prototypes()
    for n, twin in TWINS.items():
        assert n in protos, f"{n} is not declared in ins_hip.h"
        # the same argument order and names; every double becomes a float, the stepper handle the Float32 one
        want = [a.replace("double", "float").replace("ins_rk_t*", "ins_rk32_t*") for a in protos[twin]]
        assert protos[n] == want, (n, protos[n], want)
    assert protos["ins_smagtensor_f32"] == ["const ins_grid_t* grid", "float theta", "const float* u", "float* sigma", "void* stream"]
    assert protos["ins_rk_set_closure_f32"] == ["ins_rk32_t* rk", "int32_t kind", "float theta"]
    assert protos["ins_rk_set_bodyforce_f32"] == ["ins_rk32_t* rk", "const float* force"]


def test_each_entry_cites_the_reference():
    """Like its fp64 twin, every new declaration carries a comment with reference line numbers (operators.jl / setup.jl / step_explicit_runge_kutta.jl)."""
    src = open(HEADER).read()
    for n in TWINS:
        at = src.index(f"int {n}(")
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"(operators|setup|step_explicit_runge_kutta)\.jl:\d+", comment), n


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    protos = _prototypes()
    for n in TWINS:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [_ctype(p) for p in protos[n]], (n, args, protos[n])
    for f in ("smagtensor32_", "smagorinsky_force32_", "smagorinsky_closure32"):
        assert callable(getattr(ins_amd.f32, f))
    import inspect

    for f in ("timestep32_", "timesteps32_"):
        assert "θ" in inspect.signature(getattr(ins_amd.f32, f)).parameters


def test_null_arguments_and_bad_kind_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    for call in (lambda: lib.ins_smagtensor_f32(None, 0.17, None, None, None),
                 lambda: lib.ins_smagorinsky_force_f32(None, 0.17, None, None, None, None),
                 lambda: lib.ins_rk_set_closure_f32(None, 1, 0.17),
                 lambda: lib.ins_rk_set_bodyforce_f32(None, None)):
        assert call() == -1
        assert b"null" in lib.ins_last_error()
    # a bad kind is refused before the handle is looked at
    for kind in (2, -1):
        assert lib.ins_rk_set_closure_f32(None, kind, 0.17) == -1
        assert b"kind" in lib.ins_last_error()
