"""CPU-side checks of the Float32 temperature equation's boundary (include/ins_hip.h, csrc/ins_temp32.hip, ins_amd.f32): the symbols are declared with
their reference citations, exported and bound; NULL handles come back as error codes; the Python entry points exist."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")

SYMBOLS = ["ins_apply_bc_temp_f32", "ins_convection_diffusion_temp_f32", "ins_dissipation_f32", "ins_gravity_f32", "ins_rk_set_temperature_f32",
           "ins_rk_step_ext_f32", "ins_rk_steps_ext_f32"]


def test_header_declares_the_symbols_with_reference_citations():
    src = open(HEADER, encoding="utf-8").read()
    assert "Float32 temperature equation" in src
    for name in SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, src, flags=re.S)
        assert m, f"{name}: no prototype with a comment in front of it"
        assert re.search(r"\w+\.jl:\d+", m.group(1)), f"{name}: its comment cites no reference lines"


def test_library_exports_and_binds_the_symbols():
    import ins_amd

    lib = ins_amd._lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), f"{name} not exported"
        assert name in ins_amd._lib.SIGNATURES, f"{name} has no ctypes signature"


def test_null_arguments_are_error_codes():
    import ins_amd

    lib = ins_amd._lib.load()
    assert lib.ins_gravity_f32(None, 0, 0.0, None, None, None) == -1
    assert b"null" in lib.ins_last_error()
    assert lib.ins_rk_step_ext_f32(None, 0.0, None, None, 0.0, None) == -1
    assert b"null" in lib.ins_last_error()
    assert lib.ins_rk_set_temperature_f32(None, None) == -1


def test_python_entry_points():
    import ins_amd

    f32 = ins_amd.f32
    for name in ("apply_bc_temp32_", "convection_diffusion_temp32_", "dissipation32_", "gravity32_", "momentum32_", "temperaturefield32"):
        assert callable(getattr(f32, name)), name
    assert "temp" in inspect.signature(f32.momentum32_).parameters
    assert "temp" in inspect.signature(f32.timestep32_).parameters
    assert "temp" in inspect.signature(f32.timesteps32_).parameters
