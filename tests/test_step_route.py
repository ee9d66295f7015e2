"""Which native entries a step calls, for every combination of the facts the steppers route on (`_step_route.py`; DESIGN.md "Step routes"), without
a device: `_lib.call` is a recorder that notes every entry name and stops the call at the first terminal entry (a native step, or the first combine of a
host stage loop), the setup is a stand-in on the CPU.  The expectations below are literals, recorded by this file's own driver on the commit BEFORE the
routes were gathered in one table (`python tests/test_step_route.py` prints them), so they pin that the table routes every case as the five modules
routed it before: same entries, same order, same setters, same exception types.

A row of TABLE is one (driver, method, INS_HOST_STAGE_LOOP, velocity boundary data, temperature); its string has one letter of OUTCOMES per
(force, closure, θ) in the order of itertools.product(FORCE, CLOSURE, THETA).  The Float32 drivers take a cache, not a method: their rows have one
method.  A closure that carries the library's marker without `_ins_setup` is not a case: nothing in the package can make one."""
import ctypes as C
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

TERMINAL = {"ins_rk_step_f64", "ins_rk_steps_f64", "ins_rk_step_bc_f64", "ins_rk_step_ext_f64", "ins_rk_step_f32", "ins_rk_steps_f32",
            "ins_rk_step_ext_f32", "ins_rk_steps_ext_f32", "ins_combine_f64"}
DRIVERS64 = ("timestep_", "timesteps_1", "timesteps_3")
DRIVERS32 = ("timestep32_", "timesteps32_")
METHOD = ("RK44", "LMWray3")
HOST = (False, True)
BC_U = ("const", "callable")
TEMP = ("none", "both", "callable", "field_only", "eq_only")  # no temperature; field and equation; with callable data; a field without an equation; vice versa
FORCE = ("none", "steady", "unsteady")
CLOSURE = ("none", "mine", "other", "user")  # the library's Smagorinsky closure of this setup / of another setup; a user callable
THETA = ("none", "scalar", "tensor")
COLUMNS = list(itertools.product(FORCE, CLOSURE, THETA))


class _Stop(Exception):
    pass


def _setup(ins, bc_u, temp, force):
    P, Dn = ins.PeriodicBC, ins.DirichletBC
    N = (4, 4)
    per = (P(), P())
    g = SimpleNamespace(N=N, dimension=2, Ip=((1, 3), (1, 3)), xp=(np.linspace(0.0, 1.0, 4),) * 2)
    s = SimpleNamespace(grid=g, device=torch.device("cpu"), Re=100.0, handle=None, stream=None, closure_model=None, temperature=None, bodyforce=None,
                        issteadybodyforce=False, needs_bc_planes=bc_u == "callable", ptr=lambda f, vector: C.c_void_p(),
                        boundary_conditions=(per, (Dn(), Dn(lambda al, x, y, t: 1.0 + 0 * x))) if bc_u == "callable" else (per, per))
    if temp in ("both", "callable", "eq_only"):
        hot = Dn((lambda x, y, t: 1.0 + 0 * x) if temp == "callable" else 1.0)
        s.temperature = SimpleNamespace(α1=0.01, α2=1.0, α3=0.1, α4=0.01, γ=1.4, gdir=1, dodissipation=True, boundary_conditions=(per, (hot, Dn(0.0))))
    if force == "steady":
        s.bodyforce, s.issteadybodyforce = ins.setup._alloc(s, N + (2,)), True
    elif force == "unsteady":
        s.bodyforce = lambda al, x, y, t: 0 * x
    return s


def _closure(ins, s, kind, make):
    if kind == "mine":
        return make(s)
    if kind == "other":
        return make(_setup(ins, "const", "none", "none"))
    return None if kind == "none" else (lambda u, θ: u)


def _theta(kind):
    return {"none": None, "scalar": 0.17, "tensor": torch.tensor(0.17, dtype=torch.float64)}[kind]


def outcome(ins, monkeypatch, driver, method, host, bc_u, temp, force, closure, theta):
    """The entry names a call of `driver` makes up to its first terminal entry, then "!Type" if it raised one of the refusal types."""
    ts, f32 = ins.time_steppers, ins.f32
    log = []

    def call(name, *args):
        log.append(name)
        if name in TERMINAL:
            raise _Stop

    monkeypatch.setattr(ins._lib, "call", call)
    monkeypatch.setattr(ts, "vectorfield", lambda setup: ins.setup._alloc(setup, setup.grid.N + (2,)))
    monkeypatch.setattr(ts, "scalarfield", lambda setup: ins.setup._alloc(setup, setup.grid.N))
    monkeypatch.setattr(ins.operators, "_bc_planes", lambda setup, t, dudt: ((C.c_void_p * 18)(), []))
    if host:
        monkeypatch.setenv("INS_HOST_STAGE_LOOP", "1")
    else:
        monkeypatch.delenv("INS_HOST_STAGE_LOOP", raising=False)
    s = _setup(ins, bc_u, temp, force)
    ps = SimpleNamespace(handle=None)
    with_field = temp in ("both", "callable", "field_only")
    try:
        if driver in DRIVERS64:
            s.closure_model = _closure(ins, s, closure, ins.smagorinsky_closure)
            if method == "LMWray3":
                m, cache = ins.LMWray3(), ts.LMWray3Cache(s, ps)
            else:
                m, cache = ins.RKMethods.RK44(), object.__new__(ts.ERKCache)
                cache.method, cache.setup, cache.psolver, cache._handle = m, s, ps, None
            st = ins.create_stepper(m, setup=s, psolver=ps, u=ins.setup._alloc(s, (4, 4, 2)), temp=ins.setup._alloc(s, (4, 4)) if with_field else None)
            if driver == "timestep_":
                ts.timestep_(m, st, 1e-3, θ=_theta(theta), cache=cache)
            else:
                ts.timesteps_(m, st, 1e-3, int(driver[-1]), θ=_theta(theta), cache=cache)
        else:
            s.closure_model = _closure(ins, s, closure, f32.smagorinsky_closure32)
            cache = object.__new__(f32.ERKCache32)
            cache.setup, cache.psolver, cache._handle = s, ps, None
            u, tf = f32.vectorfield32(s), f32.scalarfield32(s) if with_field else None
            if driver == "timestep32_":
                f32.timestep32_(cache, u, 1e-3, temp=tf, θ=_theta(theta))
            else:
                f32.timesteps32_(cache, u, 1e-3, 3, temp=tf, θ=_theta(theta))
        log.append("(returned)")  # no terminal entry: the call came back
    except _Stop:
        pass
    except (TypeError, ValueError, NotImplementedError) as e:
        log.append("!" + type(e).__name__)
    return " ".join(log)


def rows():
    for d in DRIVERS64:
        yield from itertools.product((d,), METHOD, HOST, BC_U, TEMP)
    for d in DRIVERS32:
        yield from itertools.product((d,), METHOD[:1], HOST, BC_U, TEMP)


# ---- recorded on the parent commit: letter -> entry names up to the first terminal entry ("!Type": raised before one)
OUTCOMES = {
    'A': 'ins_rk_step_f64',
    'B': 'ins_combine_f64',
    'C': 'ins_rk_set_closure ins_rk_set_temperature ins_rk_step_ext_f64',
    'D': 'ins_rk_set_bodyforce ins_rk_step_f64',
    'E': 'ins_rk_set_bodyforce ins_rk_set_closure ins_rk_set_temperature ins_rk_step_ext_f64',
    'F': '!ValueError',
    'G': 'ins_rk_step_bc_f64',
    'H': 'ins_rk_set_bodyforce ins_rk_step_bc_f64',
    'I': 'ins_rk_create ins_rk_step_f64',
    'J': 'ins_rk_create ins_rk_set_closure ins_rk_set_temperature ins_rk_step_ext_f64',
    'K': 'ins_rk_create ins_rk_set_bodyforce ins_rk_step_f64',
    'L': 'ins_rk_create ins_rk_set_bodyforce ins_rk_set_closure ins_rk_set_temperature ins_rk_step_ext_f64',
    'M': 'ins_rk_steps_f64',
    'N': 'ins_rk_set_bodyforce ins_rk_steps_f64',
    'O': 'ins_rk_create ins_rk_steps_f64',
    'P': 'ins_rk_create ins_rk_set_bodyforce ins_rk_steps_f64',
    'Q': 'ins_rk_step_f32',
    'R': '!NotImplementedError',
    'S': 'ins_rk_set_closure_f32 ins_rk_step_ext_f32',
    'T': 'ins_rk_set_bodyforce_f32 ins_rk_step_ext_f32',
    'U': 'ins_rk_set_bodyforce_f32 !NotImplementedError',
    'V': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 ins_rk_step_ext_f32',
    'W': 'ins_rk_set_temperature_f32 ins_rk_step_ext_f32',
    'X': 'ins_rk_set_closure_f32 ins_rk_set_temperature_f32 ins_rk_step_ext_f32',
    'Y': 'ins_rk_set_bodyforce_f32 ins_rk_set_temperature_f32 ins_rk_step_ext_f32',
    'Z': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 ins_rk_set_temperature_f32 ins_rk_step_ext_f32',
    'a': 'ins_rk_set_closure_f32 !NotImplementedError',
    'b': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 !NotImplementedError',
    'c': 'ins_rk_set_closure_f32 !ValueError',
    'd': 'ins_rk_set_bodyforce_f32 !ValueError',
    'e': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 !ValueError',
    'f': 'ins_rk_steps_f32',
    'g': 'ins_rk_set_closure_f32 ins_rk_steps_ext_f32',
    'h': 'ins_rk_set_bodyforce_f32 ins_rk_steps_ext_f32',
    'i': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 ins_rk_steps_ext_f32',
    'j': 'ins_rk_set_temperature_f32 ins_rk_steps_ext_f32',
    'k': 'ins_rk_set_closure_f32 ins_rk_set_temperature_f32 ins_rk_steps_ext_f32',
    'l': 'ins_rk_set_bodyforce_f32 ins_rk_set_temperature_f32 ins_rk_steps_ext_f32',
    'm': 'ins_rk_set_bodyforce_f32 ins_rk_set_closure_f32 ins_rk_set_temperature_f32 ins_rk_steps_ext_f32',
}
TABLE = {
    ('timestep_', 'RK44', False, 'const', 'none'): 'AAABCBBBBBBBDDDBEBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'const', 'both'): 'CCCBCBBBBBBBEEEBEBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', False, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', False, 'callable', 'none'): 'GGGBBBBBBBBBHHHBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', True, 'const', 'none'): 'AAABBBBBBBBBDDDBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', True, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'RK44', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'RK44', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', False, 'const', 'none'): 'IIIBJBBBBBBBKKKBLBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'const', 'both'): 'JJJBJBBBBBBBLLLBLBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', False, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', False, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', True, 'const', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', True, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timestep_', 'LMWray3', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep_', 'LMWray3', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', False, 'const', 'none'): 'MMMBCBBBBBBBNNNBEBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'const', 'both'): 'CCCBCBBBBBBBEEEBEBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', False, 'const', 'eq_only'): 'MMMFFFFFFFFFNNNFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', False, 'callable', 'none'): 'GGGBBBBBBBBBHHHBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', True, 'const', 'none'): 'MMMBBBBBBBBBNNNBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', True, 'const', 'eq_only'): 'MMMFFFFFFFFFNNNFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'RK44', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'RK44', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', False, 'const', 'none'): 'OOOBJBBBBBBBPPPBLBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'const', 'both'): 'JJJBJBBBBBBBLLLBLBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', False, 'const', 'eq_only'): 'OOOFFFFFFFFFPPPFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', False, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', True, 'const', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', True, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_1', 'LMWray3', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_1', 'LMWray3', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', False, 'const', 'none'): 'MMMBCBBBBBBBNNNBEBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'const', 'both'): 'CCCBCBBBBBBBEEEBEBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', False, 'const', 'eq_only'): 'MMMFFFFFFFFFNNNFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', False, 'callable', 'none'): 'GGGBBBBBBBBBHHHBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', True, 'const', 'none'): 'MMMBBBBBBBBBNNNBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', True, 'const', 'eq_only'): 'MMMFFFFFFFFFNNNFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'RK44', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'RK44', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', False, 'const', 'none'): 'OOOBJBBBBBBBPPPBLBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'const', 'both'): 'JJJBJBBBBBBBLLLBLBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', False, 'const', 'eq_only'): 'OOOFFFFFFFFFPPPFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', False, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', False, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', False, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', True, 'const', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'const', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'const', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'const', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', True, 'const', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', True, 'callable', 'none'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'callable', 'both'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'callable', 'callable'): 'BBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBBB',
    ('timesteps_3', 'LMWray3', True, 'callable', 'field_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timesteps_3', 'LMWray3', True, 'callable', 'eq_only'): 'FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF',
    ('timestep32_', 'RK44', False, 'const', 'none'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'const', 'both'): 'WWWRXRRRRRRRYYYUZUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'const', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'const', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'const', 'eq_only'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'callable', 'none'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'callable', 'both'): 'WWWRXRRRRRRRYYYUZUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'callable', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'callable', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', False, 'callable', 'eq_only'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'const', 'none'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'const', 'both'): 'WWWRXRRRRRRRYYYUZUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'const', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'const', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'const', 'eq_only'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'callable', 'none'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'callable', 'both'): 'WWWRXRRRRRRRYYYUZUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'callable', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'callable', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timestep32_', 'RK44', True, 'callable', 'eq_only'): 'QQQRSRRRRRRRTTTUVUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'const', 'none'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'const', 'both'): 'jjjRkRRRRRRRlllUmUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'const', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'const', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'const', 'eq_only'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'callable', 'none'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'callable', 'both'): 'jjjRkRRRRRRRlllUmUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'callable', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'callable', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', False, 'callable', 'eq_only'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'const', 'none'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'const', 'both'): 'jjjRkRRRRRRRlllUmUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'const', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'const', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'const', 'eq_only'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'callable', 'none'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'callable', 'both'): 'jjjRkRRRRRRRlllUmUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'callable', 'callable'): 'RRRRaRRRRRRRUUUUbUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'callable', 'field_only'): 'FFFRcRRRRRRRdddUeUUUUUUURRRRRRRRRRRR',
    ('timesteps32_', 'RK44', True, 'callable', 'eq_only'): 'fffRgRRRRRRRhhhUiUUUUUUURRRRRRRRRRRR',
}


@pytest.mark.parametrize("row", list(TABLE), ids=lambda r: "-".join(str(v) for v in r))
def test_entries_called_are_the_recorded_ones(row, monkeypatch):
    import ins_amd as ins

    assert len(TABLE[row]) == len(COLUMNS)
    wrong = []
    for letter, col in zip(TABLE[row], COLUMNS):
        got = outcome(ins, monkeypatch, *row, *col)
        if got != OUTCOMES[letter]:
            wrong.append((col, got, OUTCOMES[letter]))
    assert not wrong, wrong


def test_table_is_the_whole_cross_product():
    assert list(TABLE) == list(rows()) and len(TABLE) * len(COLUMNS) == 5760


if __name__ == "__main__":  # print OUTCOMES and TABLE as this tree routes them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ins_amd as ins

    letters, table = {}, {}
    mp = pytest.MonkeyPatch()
    for row in rows():
        table[row] = "".join(letters.setdefault(outcome(ins, mp, *row, *col), "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"[len(letters)])
                             for col in COLUMNS)
    mp.undo()
    print("OUTCOMES = {")
    for o, k in letters.items():
        print(f"    {k!r}: {o!r},")
    print("}\nTABLE = {")
    for row, s in table.items():
        print(f"    {row!r}: {s!r},")
    print("}")
