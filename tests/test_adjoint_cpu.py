"""CPU-side checks of the reverse-mode layer: every pullback entry point is declared in include/ins_hip.h with a reference citation and
whether it overwrites or accumulates, julia/INSHip.jl binds each, and `ins_amd.ad` imports wherever the library does."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")
GLUE = os.path.join(ROOT, "julia", "INSHip.jl")

PULLBACKS = {  # C entry -> (Julia method, what its comment must cite)
    "ins_divergence_adjoint_f64": ("divergence_adjoint!", "operators.jl:127-145"),
    "ins_pressuregradient_adjoint_f64": ("pressuregradient_adjoint!", "operators.jl:180-199"),
    "ins_convection_adjoint_f64": ("convection_adjoint!", "operators.jl:417-519"),
    "ins_diffusion_adjoint_f64": ("diffusion_adjoint!", "operators.jl:575-616"),
    "ins_momentum_pullback_f64": (None, "operators.jl:967-976"),
    "ins_apply_bc_u_pullback_f64": ("apply_bc_u_pullback!", "boundary_conditions.jl:"),
    "ins_apply_bc_p_pullback_f64": ("apply_bc_p_pullback!", "boundary_conditions.jl:"),
    "ins_project_pullback_f64": ("project_pullback!", "pressure.jl:"),
}


def test_header_declares_each_pullback_with_a_citation():
    src = open(HEADER).read()
    for name, (_, cite) in PULLBACKS.items():
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + name + r"\(", src, flags=re.S)
        assert m, f"{name} is not declared behind its own comment"
        comment = m.group(1)
        assert cite in comment, f"{name}: comment does not cite {cite}"
        assert re.search(r"\+=|overwrites|accumulate|in place", comment), f"{name}: comment does not say whether it overwrites or accumulates"


def test_julia_glue_binds_each_pullback():
    src = open(GLUE).read()
    for name, (jl, _) in PULLBACKS.items():
        assert re.search(r"ccall\(\(:" + name + r", lib\)", src), f"no ccall of {name} in julia/INSHip.jl"
        if jl:
            assert re.search(r"(?m)^(?:function\s+)?" + re.escape(jl) + r"\(", src), f"no method {jl} in julia/INSHip.jl"


def test_ad_module_imports_when_the_library_exists():
    pkg = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd")
    if not os.path.exists(os.path.join(pkg, "libinship.so")):
        pytest.skip("libinship.so is not built")
    import ins_amd

    for f in ("apply_bc_u", "apply_bc_p", "scalewithvolume", "divergence", "pressuregradient", "applypressure", "poisson", "convection",
              "diffusion", "momentum", "project", "right_hand_side", "create_right_hand_side", "timestep"):
        assert callable(getattr(ins_amd.ad, f)), f
    for f in ("divergence_adjoint_", "pressuregradient_adjoint_", "convection_adjoint_", "diffusion_adjoint_", "momentum_pullback_",
              "apply_bc_u_pullback_", "apply_bc_p_pullback_", "project_pullback_"):
        assert callable(getattr(ins_amd, f)), f
