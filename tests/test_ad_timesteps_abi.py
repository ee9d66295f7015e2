"""CPU-side checks of the native step pullback (csrc/ins_rk_adjoint.hip) and `ad.timesteps`: exported, bound with the header's signatures, and the
refusals that need no device."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ins_rk_adjoint_create", "ins_rk_adjoint_destroy", "ins_rk_step_pullback_f64"]


def _header_args(name):
    """C parameter types of `name` as include/ins_hip.h declares them, mapped to ctypes."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ins_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in ins_hip.h"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if arg.count("*") == 2 and "ins_rk_adjoint_t" in arg:
            out.append("handle**")
        elif "*" in arg:
            out.append("double*" if re.match(r"const double\* (A|c)$", arg) else "void*")
        else:
            out.append(arg.rsplit(" ", 1)[0])
    return out


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    vp, dp = C.c_void_p, ins_amd._lib.c_double_p
    ctype = {"void*": vp, "double*": dp, "handle**": C.POINTER(vp), "int": C.c_int, "double": C.c_double}
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [ctype[a] for a in _header_args(n)], (n, _header_args(n))
    assert callable(ins_amd.ad.timesteps) and "timesteps" in ins_amd.ad.__all__


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    assert lib.ins_rk_adjoint_create(None, None, 4, None, None, None) == -1
    assert b"null" in lib.ins_last_error()
    assert lib.ins_rk_step_pullback_f64(None, 1e-3, None, None, 1e-3, None, None) == -1
    assert b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_destroy(None) == 0


def test_refusals_without_gpu():
    import torch

    import ins_amd

    method = ins_amd.RKMethods.RK44()

    def stepper(dtype):
        return SimpleNamespace(setup=None, psolver=None, u=torch.zeros((4, 4, 2), dtype=dtype), temp=None, t=0.0, n=0)

    with pytest.raises(TypeError):
        ins_amd.ad.timesteps(method, stepper(torch.float32), 1e-3, 2)
    with pytest.raises(ValueError):
        ins_amd.ad.timesteps(method, stepper(torch.float64), 1e-3, 0)
    with pytest.raises(ValueError):
        ins_amd.ad.timesteps(method, stepper(torch.float64), 1e-3, 3, checkpoint_every=0)
