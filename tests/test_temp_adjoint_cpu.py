"""CPU-side checks of the temperature pullbacks: every entry point of csrc/ins_temp_adjoint.hip is declared in include/ins_hip.h behind a
comment with its reference citation and whether it overwrites, accumulates or works in place; julia/INSHip.jl binds each; `ins_amd` and
`ins_amd.ad` expose the new names wherever the library is built."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")
GLUE = os.path.join(ROOT, "julia", "INSHip.jl")

PULLBACKS = {  # C entry -> (Julia method, what its comment must cite)
    "ins_apply_bc_temp_pullback_f64": ("apply_bc_temp_pullback!", "boundary_conditions.jl:142-157"),
    "ins_gravity_adjoint_f64": ("gravity_adjoint!", "operators.jl:892-908"),
    "ins_convection_diffusion_temp_adjoint_f64": ("convection_diffusion_temp_adjoint!", "operators.jl:712-737"),
    "ins_dissipation_adjoint_f64": ("dissipation_adjoint!", "operators.jl:791-814"),
    "ins_temperature_pullback_f64": ("temperature_pullback!", "step_explicit_runge_kutta.jl:79-83"),
}


def test_header_declares_each_temperature_pullback_with_a_citation():
    src = open(HEADER).read()
    for name, (_, cite) in PULLBACKS.items():
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + name + r"\(", src, flags=re.S)
        assert m, f"{name} is not declared behind its own comment"
        comment = m.group(1)
        assert cite in comment, f"{name}: comment does not cite {cite}"
        assert re.search(r"\+=|overwrites|accumulate|in place", comment), f"{name}: comment does not say whether it overwrites or accumulates"


def test_kernel_file_is_built_and_cites_the_reference():
    csrc = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd", "csrc")
    src = open(os.path.join(csrc, "ins_temp_adjoint.hip")).read()
    assert "ins_temp_adjoint.hip" in open(os.path.join(csrc, "Makefile")).read()
    for name, (_, cite) in PULLBACKS.items():
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
    for cite in ("operators.jl:892-908", "operators.jl:712-737", "operators.jl:791-814", "boundary_conditions.jl:142-157"):
        assert cite in src, cite
    assert "atomic" not in src.replace("no atomics", "")  # gather form


def test_julia_glue_binds_each_temperature_pullback():
    src = open(GLUE).read()
    for name, (jl, _) in PULLBACKS.items():
        assert re.search(r"ccall\(\(:" + name + r", lib\)", src), f"no ccall of {name} in julia/INSHip.jl"
        assert re.search(r"(?m)^(?:function\s+)?" + re.escape(jl) + r"\(", src), f"no method {jl} in julia/INSHip.jl"


def test_python_layers_expose_the_new_names():
    pkg = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd")
    if not os.path.exists(os.path.join(pkg, "libinship.so")):
        pytest.skip("libinship.so is not built")
    import ins_amd

    for f in ("apply_bc_temp", "gravity", "convection_diffusion_temp", "dissipation", "momentum", "timestep"):
        assert callable(getattr(ins_amd.ad, f)), f
        assert f in ins_amd.ad.__all__, f
    for f in ("apply_bc_temp_pullback_", "gravity_adjoint_", "convection_diffusion_temp_adjoint_", "dissipation_adjoint_", "temperature_pullback_"):
        assert callable(getattr(ins_amd, f)), f
    for name in PULLBACKS:
        assert name in ins_amd._lib.SIGNATURES and hasattr(ins_amd._lib.load(), name), name


def test_null_arguments_come_back_as_codes():
    pkg = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd")
    if not os.path.exists(os.path.join(pkg, "libinship.so")):
        pytest.skip("libinship.so is not built")
    import ins_amd

    lib = ins_amd._lib.load()
    assert lib.ins_apply_bc_temp_pullback_f64(None, None, None, None) == -1
    assert lib.ins_gravity_adjoint_f64(None, 0, 1.0, None, None, None) == -1
    assert lib.ins_convection_diffusion_temp_adjoint_f64(None, 1.0, None, None, None, None, None, None) == -1
    assert lib.ins_dissipation_adjoint_f64(None, 1.0, 1.0, None, None, None, None) == -1
    assert lib.ins_temperature_pullback_f64(None, None, 1.0, None, None, None, None, None, None, None) == -1
