"""CPU-side checks of the differentiable tensor-basis closure: the five entries are declared in include/ins_hip.h behind a citing comment
that says whether they overwrite or accumulate, julia/INSHip.jl binds each, the Python layers expose the new callables, the new sources hold
none of the instructions the shared GPU machines forbid, and the test helper's restatement of the pointwise basis is pinned to the oracle."""
import os
import re

import numpy as np
import pytest

from tests import fixtures as fx
from tests import tensorbasis_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ins_hip.h")
GLUE = os.path.join(ROOT, "julia", "INSHip.jl")
PKG = os.path.join(ROOT, "incompressiblenavierstokes.jl_amd")

ENTRIES = {  # C entry -> (Julia method, what its comment must cite)
    "ins_tensorbasis_pullback_f64": ("tensorbasis_pullback!", "tensorbasis.jl:30-95"),
    "ins_divoftensor_adjoint_f64": ("divoftensor_adjoint!", "operators.jl:1186-1287"),
    "ins_tensorinvariants_f64": ("tensorinvariants!", "tensorbasis.jl:"),
    "ins_tensorclosure_stress_f64": ("tensorclosure_stress!", "tensorbasis.jl:"),
    "ins_tensorclosure_pullback_f64": ("tensorclosure_pullback!", "tensorbasis.jl:"),
}
NEW_SOURCES = [
    os.path.join(PKG, "csrc", "ins_tensorclosure.hip"),
    os.path.join(ROOT, "tests", "tensorbasis_ref.py"),
    os.path.join(ROOT, "tests", "test_tensorclosure_cpu.py"),
    os.path.join(ROOT, "tests", "test_gpu_tensorclosure.py"),
    os.path.join(ROOT, "tools", "tensorclosure_time.py"),
]


def test_header_declares_each_entry_with_a_citation():
    src = open(HEADER).read()
    for name, (_, cite) in ENTRIES.items():
        m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + name + r"\(", src, flags=re.S)
        assert m, f"{name} is not declared behind its own comment"
        comment = m.group(1)
        assert cite in comment, f"{name}: comment does not cite {cite}"
        assert re.search(r"\+=|overwrit|accumulate|added to", comment), f"{name}: comment does not say whether it overwrites or accumulates"


def test_julia_glue_binds_each_entry():
    src = open(GLUE).read()
    for name, (jl, _) in ENTRIES.items():
        assert re.search(r"ccall\(\(:" + name + r", lib\)", src), f"no ccall of {name} in julia/INSHip.jl"
        assert re.search(r"(?m)^(?:function\s+)?" + re.escape(jl) + r"\(", src), f"no method {jl} in julia/INSHip.jl"


def test_ctypes_table_declares_each_entry():
    src = open(os.path.join(PKG, "_lib.py")).read()
    for name in ENTRIES:
        assert f'"{name}"' in src, name


def test_python_layers_expose_the_new_callables():
    if not os.path.exists(os.path.join(PKG, "libinship.so")):
        pytest.skip("libinship.so is not built")
    import ins_amd

    for f in ("tensorbasis", "divoftensor", "lastdimcontract", "tensorinvariants", "tensorclosure_stress", "smagorinsky_closure"):
        assert callable(getattr(ins_amd.ad, f)), f
    for f in ("tensorbasis_pullback_", "divoftensor_adjoint_", "tensorinvariants_", "tensorclosure_stress_", "tensorclosure_pullback_"):
        assert callable(getattr(ins_amd, f)), f
    assert callable(ins_amd.neuralclosure.tensorclosure) and callable(ins_amd.tensorclosure)


def test_new_sources_hold_no_forbidden_instruction():
    """Scalar stores / scalar read-modify-write / scalar cache write-back instructions, and any atomic operation at all (the pullbacks are
    gather kernels).  The words are assembled here so that this file does not contain them."""
    s = "s_"
    words = [s + "store", s + "buffer_" + "store", s + "scratch_" + "store", s + "ato" + "mic", s + "buffer_" + "ato" + "mic", s + "dcache_" + "wb",
             s + "dcache_" + "discard", "ato" + "micAdd", "ato" + "micCAS", "ato" + "mic_", "__hip_" + "ato" + "mic", "unsafeAto" + "micAdd"]
    for path in NEW_SOURCES:
        assert os.path.exists(path), path
        text = open(path).read().lower()
        for w in words:
            assert w.lower() not in text, (os.path.relpath(path, ROOT), w)


@pytest.mark.parametrize("name", ["setup2d", "setup3d", "mixed"])
def test_pointwise_restatement_matches_the_oracle(oracle, name):
    """(S, R) -> (B, V) in torch after oracle.gradu equals oracle.tensorbasis: relative max-norm per tensor <= 1e-13 (the same expressions in
    the same precision)."""
    so = {"setup2d": fx.setup2d, "setup3d": fx.setup3d, "mixed": fx.setup_mixed}[name](oracle)
    g = so.grid
    u = fx.randn_field(tuple(g.N) + (g.D,), 70)
    Bref, Vref = oracle.tensorbasis(u, so)
    B, V = tr.forward(oracle, so, u)
    errs = [tr.relmax(B[..., i, :, :], Bref[..., i, :, :]) for i in range(B.shape[-3])] + [tr.relmax(V[..., i], Vref[..., i]) for i in range(V.shape[-1])]
    print(name, "relative max-norm errors per tensor:", " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-13, errs
    # the layout converters are inverse to each other
    assert np.array_equal(tr.oracle_B_from_lib(tr.lib_B_from_oracle(Bref), g.D), Bref)
