"""The carry plan of csrc/ins_rk_terms.h (RkCarryPlan) without a device.  In the stage-velocity basis the last stage i of RK44 forms
    V_3 = c0 ustart + β_0 V_0 + β_1 V_1 + β_2 V_2 + Δt A[3,3] k_3,      c0 = 1 - Σβ = -1/3,  β = (1/3, 2/3, 1/3);
with the plan stage j = 1 stores S = a0 s + a1 V_0 + a2 V_1 (s = ustart, plus Δt A[1,1] f with a steady body force f) and stage 3 forms
S + β_2 V_2 + cf' f + Δt A[3,3] k_3.  Checked here, for every tableau of RKMethods:
  * RK44 has the plan (j, i) = (1, 3) and a = (c0, β_0, β_1) bit for bit as ins_rk_stage_terms solves them, within one ulp of -1/3, 1/3, 2/3;
  * where a plan exists, its terms expanded back over (ustart, V_m, f, k_i) reproduce the unplanned combination of ins_rk_stage_terms: the coefficients of
    ustart, of every V_m and of k_i exactly (rational arithmetic on the doubles), the body force's within two ulps of the largest number its two products
    and one difference pass through (each of the three operations rounds once, to half an ulp of a number no larger than that);
  * Wray3, SSP33 and FE11 have no plan."""
import ctypes as C
import inspect
from fractions import Fraction

import numpy as np
import pytest

MAX_STAGES = 16  # INS_MAX_STAGES of csrc/ins_internal.h
DTS = (1e-3, 0.37)


def methods():
    import ins_amd as ins

    return [n for n, f in inspect.getmembers(ins.RKMethods, inspect.isfunction) if not n.startswith("_")]


METHODS = methods()


def tableau(name):
    import ins_amd as ins

    return np.ascontiguousarray(getattr(ins.RKMethods, name)().A, dtype=np.float64)


def plan(A, dt, force):
    from ins_amd import _lib

    fn = _lib.load().ins_dbg_rk_carry_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_double, C.c_int32] + [C.c_void_p] * 6
    j, i = C.c_int32(-7), C.c_int32(-7)
    a = (C.c_double * 3)()
    self_in, coef_self, cforce = C.c_double(), C.c_double(), C.c_double()
    rc = fn(len(A), A.ctypes.data, dt, int(force), C.addressof(j), C.addressof(i), C.addressof(a), C.addressof(self_in), C.addressof(coef_self),
            C.addressof(cforce))
    assert rc == 0
    return dict(j=j.value, i=i.value, a=tuple(a), self_in=self_in.value, coef_self=coef_self.value, cforce=cforce.value)


def unplanned(A, i, dt, force):
    """ins_rk_stage_terms in the stage-velocity basis with the stencil input in registers, as rk_step_fused_periodic calls it"""
    from ins_amd import _lib

    fn = _lib.load().ins_dbg_rk_stage_terms
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    n, write_k = C.c_int32(-1), C.c_int32(-1)
    stage = (C.c_int32 * (MAX_STAGES + 1))()
    coef = (C.c_double * (MAX_STAGES + 1))()
    c0m1, self_in, coef_self, cforce = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    rc = fn(len(A), A.ctypes.data, i, dt, 1, 1, int(force), 0, C.addressof(n), C.addressof(stage), C.addressof(coef), C.addressof(c0m1),
            C.addressof(self_in), C.addressof(coef_self), C.addressof(write_k), C.addressof(cforce))
    assert rc == 0
    return dict(terms=[(stage[q], coef[q]) for q in range(n.value)], c0m1=c0m1.value, self_in=self_in.value, coef_self=coef_self.value, cforce=cforce.value)


def test_rk44_plan():
    A = tableau("RK44")
    for dt in DTS:
        p = plan(A, dt, False)
        assert (p["j"], p["i"]) == (1, 3)
        u = unplanned(A, 3, dt, False)
        assert u["terms"] == [(0, p["a"][1]), (1, p["a"][2])]  # the loaded terms the plan replaces, bit for bit
        assert p["a"][0] == 1.0 + u["c0m1"]
        assert p["self_in"] == u["self_in"] and p["coef_self"] == u["coef_self"]
        for got, want in zip(p["a"], (-1.0 / 3.0, 1.0 / 3.0, 2.0 / 3.0)):
            assert abs(got - want) <= np.spacing(abs(want))


@pytest.mark.parametrize("name", ["Wray3", "SSP33", "FE11"])
def test_short_methods_have_no_plan(name):
    p = plan(tableau(name), 1e-3, True)
    assert p["j"] < 0 and p["i"] < 0


@pytest.mark.parametrize("force", [False, True], ids=["noforce", "force"])
@pytest.mark.parametrize("name", METHODS)
def test_planned_terms_expand_to_the_unplanned_combination(name, force):
    A = tableau(name)
    ns = len(A)
    if any(A[m, m] == 0.0 for m in range(ns)):
        for dt in DTS:
            assert plan(A, dt, force)["j"] < 0  # no stage-velocity basis, no plan
        return
    for dt in DTS:
        p = plan(A, dt, force)
        if p["j"] < 0:
            assert p["i"] < 0
            continue
        j, i = p["j"], p["i"]
        assert 1 <= j and j + 2 == i == ns - 1
        # the producing stage's s is ustart (times exactly 1) plus the force's share; the stage between does not read what the plan displaces
        uj = unplanned(A, j, dt, force)
        assert uj["c0m1"] == 0.0 and uj["self_in"] == 0.0 and [s for s, _ in uj["terms"] if s < ns] == []
        assert all(s != j - 1 for s, _ in unplanned(A, j + 1, dt, force)["terms"])
        u = unplanned(A, i, dt, force)
        # coefficients over (ustart, V_0 .. V_{i-1}, k_i) as exact rationals of the doubles
        want = {"ustart": Fraction(1.0 + u["c0m1"]), "k": Fraction(u["coef_self"]), i - 1: Fraction(u["self_in"])}
        for s, c in u["terms"]:
            if s < ns:
                want[s] = want.get(s, 0) + Fraction(c)
        got = {"ustart": Fraction(p["a"][0]), "k": Fraction(p["coef_self"]), i - 1: Fraction(p["self_in"])}
        got[j - 1] = got.get(j - 1, 0) + Fraction(p["a"][1])
        got[j] = got.get(j, 0) + Fraction(p["a"][2])
        assert {k: v for k, v in got.items() if v != 0} == {k: v for k, v in want.items() if v != 0}
        if force:
            # S holds a0·(Δt A[j,j]) f through the producing stage's s; the consuming stage's own coefficient makes up the difference
            share = Fraction(p["a"][0]) * Fraction(uj["cforce"])
            total = Fraction(p["cforce"]) + share
            scale = max(abs(u["cforce"]), abs(float(share)), abs(p["cforce"]))
            assert abs(total - Fraction(u["cforce"])) <= 2 * Fraction(float(np.spacing(scale)))
        else:
            assert p["cforce"] == 0.0 and u["cforce"] == 0.0
