"""CPU-side checks of the ensemble stepper (csrc/ins_rk_ensemble.hip; `EnsembleCache`, `timesteps_ensemble_`, `vectorfields`): the three symbols are in
include/ins_hip.h, exported and bound with the header's argument lists; the argument errors of the C entries that need no device; and the refusals of the
Python functions, every one of which comes before a setup, a solver or the device is touched."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ins_rk_ensemble_create", "ins_rk_ensemble_destroy", "ins_rk_ensemble_steps_f64"]


def _header_args(name):
    """C parameter types of `name` as include/ins_hip.h declares them, mapped to ctypes names."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ins_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in ins_hip.h"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if arg.count("*") == 2:
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
    ctype = {"void*": vp, "double*": dp, "handle**": C.POINTER(vp), "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [ctype[a] for a in _header_args(n)], (n, _header_args(n))
    assert _header_args("ins_rk_ensemble_create") == ["void*", "void*", "int", "double*", "double*", "int", "handle**"]
    assert _header_args("ins_rk_ensemble_steps_f64") == ["void*", "double", "void*", "int64_t", "double", "double", "int", "void*"]
    assert callable(ins_amd.vectorfields) and callable(ins_amd.timesteps_ensemble_) and isinstance(ins_amd.EnsembleCache, type)


def test_argument_errors_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    INVALID = -1
    # null handles
    assert lib.ins_rk_ensemble_create(None, None, 4, None, None, 3, None) == INVALID and b"null" in lib.ins_last_error()
    assert lib.ins_rk_ensemble_steps_f64(None, 1e-3, None, 0, 0.0, 1e-3, 1, None) == INVALID and b"null" in lib.ins_last_error()
    assert lib.ins_rk_ensemble_destroy(None) == 0
    # the checks both entries make once they know the grid's ncell (the hook calls the function they call)
    args = lib.ins_dbg_rk_ensemble_args
    args.restype, args.argtypes = C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_int32]
    ncell = 18 * 34
    assert args(ncell, 3, 2 * ncell, 5) == 0 and args(ncell, 1, 2 * ncell + 7, 0) == 0
    assert args(ncell, 0, 2 * ncell, 5) == INVALID and b"members" in lib.ins_last_error()
    assert args(ncell, -2, 2 * ncell, 5) == INVALID and b"members" in lib.ins_last_error()
    assert args(ncell, 3, 2 * ncell, -1) == INVALID and b"steps" in lib.ins_last_error()
    assert args(ncell, 3, 2 * ncell - 1, 5) == INVALID and b"stride" in lib.ins_last_error()


# ------------------------------------------------------------------------------------ refusals of the Python functions
def _untouchable():
    """A stand-in for a setup / solver handle: any use of it is an error."""

    class H:
        def __getattr__(self, name):
            raise AssertionError(f"the refusal must come before the setup is touched (.{name})")

    return H()


def _cache(N=(18, 34), B=3):
    """An EnsembleCache without a handle: what `timesteps_ensemble_` checks of U needs the grid's shape, B and the device only."""
    import ins_amd as ins

    c = object.__new__(ins.EnsembleCache)
    c.setup = SimpleNamespace(grid=SimpleNamespace(N=N, dimension=2), device=torch.device("cpu"), handle=_untouchable(), Re=_untouchable(), stream=_untouchable())
    c.B, c._handle = B, None
    return c


def _members(B, N, dtype=torch.float64):
    shape = N + (2,)
    return torch.zeros((B,) + tuple(reversed(shape)), dtype=dtype).permute(0, 3, 2, 1)


def test_python_refusals_of_the_field_without_gpu():
    import ins_amd as ins

    N, B = (18, 34), 3
    c = _cache(N, B)
    good = _members(B, N)
    assert tuple(good.shape) == (B,) + N + (2,) and tuple(good[1].stride()) == (1, N[0], N[0] * N[1])
    with pytest.raises(TypeError, match="float64"):
        ins.timesteps_ensemble_(c, _members(B, N, torch.float32), 0.0, 1e-3, 2)
    with pytest.raises(TypeError, match="float64"):
        ins.timesteps_ensemble_(c, [good[0], good[1], good[2]], 0.0, 1e-3, 2)
    with pytest.raises(TypeError, match="EnsembleCache"):
        ins.timesteps_ensemble_(SimpleNamespace(), good, 0.0, 1e-3, 2)
    for bad in (good[0], _members(B, (18, 18)), torch.zeros((B,) + N + (3,), dtype=torch.float64), good[..., 0]):
        with pytest.raises(ValueError, match="shape"):
            ins.timesteps_ensemble_(c, bad, 0.0, 1e-3, 2)
    with pytest.raises(ValueError, match="B = 3"):
        ins.timesteps_ensemble_(c, _members(B + 1, N), 0.0, 1e-3, 2)
    with pytest.raises(ValueError, match="column-major"):  # C-ordered members
        ins.timesteps_ensemble_(c, torch.zeros((B,) + N + (2,), dtype=torch.float64), 0.0, 1e-3, 2)
    with pytest.raises(ValueError, match="overlap"):  # the same member B times
        ins.timesteps_ensemble_(c, good[:1].expand(B, -1, -1, -1), 0.0, 1e-3, 2)
    with pytest.raises(ValueError, match="nsteps"):
        ins.timesteps_ensemble_(c, good, 0.0, 1e-3, -1)
    with pytest.raises(ValueError, match="at least one member"):
        ins.vectorfields(SimpleNamespace(grid=SimpleNamespace(N=N, dimension=2), device=_untouchable()), 0)


def _setup(**kw):
    from ins_amd.boundary_conditions import PeriodicBC

    d = dict(temperature=None, closure_model=None, bodyforce=None, issteadybodyforce=False, needs_bc_planes=False,
             boundary_conditions=((PeriodicBC(), PeriodicBC()),) * 2, grid=SimpleNamespace(N=(34, 34), dimension=2), device=torch.device("cpu"),
             handle=_untouchable())
    d.update(kw)
    return SimpleNamespace(**d)


def test_python_refusals_of_the_problem_without_gpu():
    """Everything outside the chained 2-D loop is refused with the per-member route named, before the library is asked for a handle."""
    import ins_amd as ins
    from ins_amd.boundary_conditions import DirichletBC, PeriodicBC

    ps = object.__new__(ins.psolver_spectral)
    rk44, fe11 = ins.RKMethods.RK44(), ins.RKMethods.FE11()
    per = (PeriodicBC(), PeriodicBC())
    refused = [
        (rk44, _setup(grid=SimpleNamespace(N=(34, 34, 34), dimension=3), boundary_conditions=(per,) * 3), ps, "3-D"),
        (rk44, _setup(boundary_conditions=(per, (DirichletBC(), DirichletBC()))), ps, "not periodic"),
        (rk44, _setup(grid=SimpleNamespace(N=(50, 34), dimension=2)), ps, "48 x 32"),
        (rk44, _setup(grid=SimpleNamespace(N=(10, 34), dimension=2)), ps, "8 x 32"),
        (rk44, _setup(bodyforce=torch.zeros(34, 34, 2), issteadybodyforce=True), ps, "body force"),
        (rk44, _setup(closure_model=lambda u, θ: u), ps, "closure"),
        (rk44, _setup(temperature=SimpleNamespace()), ps, "temperature"),
        (fe11, _setup(), ps, "one-stage"),
        (rk44, _setup(), object.__new__(ins.psolver_cg), "psolver_cg"),
    ]
    for method, sp, solver, what in refused:
        with pytest.raises(NotImplementedError, match=what) as e:
            ins.EnsembleCache(method, sp, solver, 4)
        assert "timesteps_" in str(e.value) and "per member" in str(e.value)
    with pytest.raises(ValueError, match="at least one member"):
        ins.EnsembleCache(rk44, _setup(), ps, 0)
