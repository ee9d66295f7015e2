"""CPU-side checks of the Float32 driver entry points (csrc/ins_fields32.hip, csrc/ins_spectrum.hip): declared in include/ins_hip.h as the float twins
of their fp64 namesakes, bound in `_lib.py` with matching argument types, exported by the built library, argument errors come back as codes without
a device, and `solve_unsteady` refuses mixed precisions before anything is launched."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

# new entry -> its fp64 twin
TWINS = {
    "ins_cfl_timestep_f32": "ins_cfl_timestep_f64",
    "ins_vorticity_f32": "ins_vorticity_f64",
    "ins_interpolate_u_p_f32": "ins_interpolate_u_p_f64",
    "ins_interpolate_w_p_f32": "ins_interpolate_w_p_f64",
    "ins_qfield_f32": "ins_qfield_f64",
    "ins_spectrum_f32": "ins_spectrum_f64",
}


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ins_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        out[m.group(1)] = [" ".join(a.split()) for a in m.group(2).split(",")]
    return out


def _ctype(param):
    """The ctypes type `_lib.py` binds a C parameter declaration with (a scalar result comes back through a typed pointer, as in the fp64 twin)."""
    if param == "float* out":
        return C.POINTER(C.c_float)
    t = re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", param).strip()  # drop the parameter name
    if t.endswith("*"):
        return C.c_void_p
    return {"int": C.c_int, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double}[t]


def test_declared_as_float_twins_of_the_f64_entries():
    protos = _prototypes()
    for n, twin in TWINS.items():
        assert n in protos, f"{n} is not declared in ins_hip.h"
        # the same argument order and names; the field arguments become float (the spectrum stays a double vector: only its gather reads floats)
        want = [a if a == "double* ehat" else a.replace("double", "float") for a in protos[twin]]
        assert protos[n] == want, (n, protos[n], want)
    assert protos["ins_cfl_timestep_f32"] == ["const ins_grid_t* grid", "float Re", "const float* u", "float* out", "void* stream"]
    assert protos["ins_spectrum_f32"] == ["ins_spectrum_t* spectrum", "const float* u", "double* ehat", "void* stream"]


def test_each_entry_cites_the_reference():
    """Like its fp64 twin, every new declaration carries a comment with reference line numbers (solver.jl / operators.jl / processors.jl)."""
    src = open(HEADER).read()
    for n in TWINS:
        at = src.index(f"int {n}(")
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"(operators|solver|processors)\.jl:\d+", comment), n


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
    for f in ("get_cfl_timestep32_", "vorticity32_", "interpolate_u_p32_", "interpolate_ω_p32_", "Qfield32_"):
        assert callable(getattr(ins_amd.f32, f))


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    for call in (lambda: lib.ins_cfl_timestep_f32(None, 1000.0, None, None, None),
                 lambda: lib.ins_vorticity_f32(None, None, None, None),
                 lambda: lib.ins_interpolate_u_p_f32(None, None, None, None),
                 lambda: lib.ins_interpolate_w_p_f32(None, None, None, None),
                 lambda: lib.ins_qfield_f32(None, None, None, None),
                 lambda: lib.ins_spectrum_f32(None, None, None, None)):
        assert call() == -1
        assert b"null" in lib.ins_last_error()


def test_solve_unsteady_refuses_mixed_precisions_before_any_launch():
    """A solver, cache or temperature of the other precision is a TypeError, raised before the setup is touched (setup=None here: no device)."""
    import ins_amd as ins

    f32 = ins.f32
    u32, u64 = torch.zeros(4, 4, 2, dtype=torch.float32), torch.zeros(4, 4, 2, dtype=torch.float64)
    t32, t64 = torch.zeros(4, 4, dtype=torch.float32), torch.zeros(4, 4, dtype=torch.float64)
    # instances without a native handle: only their class is looked at
    ps32, ps64 = object.__new__(f32.psolver_spectral32), object.__new__(ins.psolver_spectral)
    wrap32 = object.__new__(f32.psolver_wrap32)
    c32, c64 = object.__new__(f32.ERKCache32), object.__new__(ins.time_steppers.ERKCache)
    kw = dict(setup=None, tlims=(0.0, 1.0), Δt=0.1)
    for bad in (dict(ustart=u32, psolver=ps64), dict(ustart=u32, cache=c64), dict(ustart=u32, tempstart=t64),
                dict(ustart=u64, psolver=ps32), dict(ustart=u64, psolver=wrap32), dict(ustart=u64, cache=c32), dict(ustart=u64, tempstart=t32)):
        with pytest.raises(TypeError, match="float32"):
            ins.solve_unsteady(**kw, **bad)


def test_solve_unsteady_refuses_lmwray3_on_float32_fields():
    import ins_amd as ins

    with pytest.raises(NotImplementedError, match="LMWray3"):
        ins.solve_unsteady(setup=None, tlims=(0.0, 1.0), Δt=0.1, ustart=torch.zeros(4, 4, 2, dtype=torch.float32), method=ins.LMWray3())


def test_get_scale_numbers_refuses_float32_fields():
    import ins_amd as ins

    with pytest.raises(TypeError, match="float64"):
        ins.get_scale_numbers(torch.zeros(4, 4, 2, dtype=torch.float32), None)
