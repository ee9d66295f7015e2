"""CPU-side checks of the Float32 pullback entry points (csrc/ins_adjoint32.hip): exported, bound, and argument errors come back as codes
without a device."""
import ctypes as C

NAMES = [
    "ins_divergence_adjoint_f32",
    "ins_pressuregradient_adjoint_f32",
    "ins_momentum_pullback_f32",
    "ins_apply_bc_u_pullback_f32",
    "ins_apply_bc_p_pullback_f32",
    "ins_project_pullback_f32",
]


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
    assert ins_amd._lib.SIGNATURES["ins_momentum_pullback_f32"][1][1] is C.c_float  # visc is a float, unlike the _f64 twin's double
    for f in ("divergence_adjoint32_", "pressuregradient_adjoint32_", "momentum_pullback32_", "apply_bc_u_pullback32_", "apply_bc_p_pullback32_",
              "project_pullback32_"):
        assert callable(getattr(ins_amd.f32, f))
    assert ins_amd.ad32.__all__ == ["apply_bc_u", "momentum", "project", "timestep"]


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    calls = [
        lambda: lib.ins_divergence_adjoint_f32(None, None, None, None),
        lambda: lib.ins_pressuregradient_adjoint_f32(None, None, None, None),
        lambda: lib.ins_momentum_pullback_f32(None, 0.0, None, None, None, 0, None),
        lambda: lib.ins_apply_bc_u_pullback_f32(None, None, None),
        lambda: lib.ins_apply_bc_p_pullback_f32(None, None, None),
        lambda: lib.ins_project_pullback_f32(None, None, None, None, None),
    ]
    for call in calls:
        assert call() == -1
        assert b"null" in lib.ins_last_error()
