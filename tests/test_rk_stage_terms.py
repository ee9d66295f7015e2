"""The Runge-Kutta stage-term builders (csrc/ins_rk_terms.h) without a device: for every tableau of RKMethods, every stage and every combination of basis,
input-from-registers, body force and force-sum order, the terms are bit for bit those of the loops the stage drivers carried before the builder existed,
restated here in the same operation order (host code is built without fused multiply-add, so the same order gives the same bits)."""
import ctypes as C
import inspect
import itertools
import math
import struct

import numpy as np

MAX_STAGES = 16  # INS_MAX_STAGES of csrc/ins_internal.h
K_BASIS, V_BASIS, SUM_F64, SUM_F32 = range(4)
DIAG_FIRST, INDEX_ORDER = 0, 1
DTS = (1e-3, 0.37)  # neither is a power of two: every product rounds


def methods():
    import ins_amd as ins

    names = [n for n, f in inspect.getmembers(ins.RKMethods, inspect.isfunction) if not n.startswith("_")]
    assert {"FE11", "RK44", "Wray3", "SSP33", "SSP104", "DOPRI6"} <= set(names)
    return names


METHODS = methods()


def tableau(name):
    """The shifted tableau exactly as ERKCache hands it to ins_rk_create."""
    import ins_amd as ins

    A = np.ascontiguousarray(getattr(ins.RKMethods, name)().A, dtype=np.float64)
    assert A.shape[0] == A.shape[1] <= MAX_STAGES
    return A


def built(A, i, dt, kind, in_regs=False, force=False, order=DIAG_FIRST):
    from ins_amd import _lib

    fn = _lib.load().ins_dbg_rk_stage_terms
    fn.restype = C.c_int
    fn.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    n, write_k = C.c_int32(-1), C.c_int32(-1)
    stage = (C.c_int32 * (MAX_STAGES + 1))()
    coef = (C.c_double * (MAX_STAGES + 1))()
    c0m1, self_in, coef_self, cforce = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    rc = fn(len(A), A.ctypes.data, i, dt, kind, int(in_regs), int(force), order, C.addressof(n), C.addressof(stage), C.addressof(coef), C.addressof(c0m1),
            C.addressof(self_in), C.addressof(coef_self), C.addressof(write_k), C.addressof(cforce))
    assert rc == 0
    assert 0 <= n.value <= MAX_STAGES + 1
    return dict(terms=[(stage[q], coef[q]) for q in range(n.value)], c0m1=c0m1.value, self_in=self_in.value, coef_self=coef_self.value,
                write_k=write_k.value, cforce=cforce.value)


def parent_loops(A, i, dt, vbasis, in_regs, force, order):
    """The stage loops of rk_step_fused_periodic / rk_step_fused_periodic_2d / rk_step_any / ins_rk_step_ext_f64 / rk32_step before the builder, operation by
    operation.  (A stage-velocity basis with the index-order force sum ran nowhere: it is 0 + Δt A[i,i].)"""
    ns = len(A)
    a = [[float(x) for x in row] for row in A]
    terms, c0m1, self_in, write_k = [], 0.0, 0.0, 0
    if vbasis:
        beta = [0.0] * ns
        for m in range(i - 1, -1, -1):
            v = a[i][m]
            for j in range(m + 1, i):
                v -= beta[j] * a[j][m]
            beta[m] = v / a[m][m]
        for m in range(i):
            if beta[m] == 0.0:
                continue
            c0m1 -= beta[m]
            if m == i - 1 and in_regs:
                self_in = beta[m]
                continue
            terms.append((m, beta[m]))
    else:
        for j in range(i):
            coef = dt * a[i][j]
            if coef == 0.0:
                continue
            terms.append((j, coef))
        for i2 in range(i + 1, ns):
            if a[i2][i] != 0.0:
                write_k = 1
    cf = 0.0
    if force:
        if order == DIAG_FIRST:
            cf = dt * a[i][i]
            if not vbasis:
                for j in range(i):
                    cf += dt * a[i][j]
        else:
            cf = 0.0
            for j in range(i if vbasis else 0, i + 1):
                cf += dt * a[i][j]
        terms.append((ns, cf))
    return dict(terms=terms, c0m1=c0m1, self_in=self_in, coef_self=dt * a[i][i], write_k=write_k, cforce=cf)


def bits(x):
    return struct.pack("<d", x)


def assert_same_bits(got, want, what):
    assert [s for s, _ in got["terms"]] == [s for s, _ in want["terms"]], what
    for (s, cg), (_, cw) in zip(got["terms"], want["terms"]):
        assert bits(cg) == bits(cw), (what, s, cg, cw)
    for key in ("c0m1", "self_in", "coef_self", "cforce"):
        assert bits(got[key]) == bits(want[key]), (what, key, got[key], want[key])
    assert got["write_k"] == want["write_k"], what


def vbasis_possible(A):
    return bool(np.all(np.diag(A) != 0.0))


def combos(A):
    for i, dt, vbasis, in_regs, force, order in itertools.product(range(len(A)), DTS, (False, True), (False, True), (False, True),
                                                                  (DIAG_FIRST, INDEX_ORDER)):
        if vbasis and not vbasis_possible(A):
            continue
        yield i, dt, vbasis, in_regs, force, order


# (one test over all methods, not one per method: the suite's per-test fixtures cost more than a method's few hundred cases)
def test_stage_terms_are_the_parent_loops_bit_for_bit():
    for name in METHODS:
        A = tableau(name)
        ncases = 0
        for i, dt, vbasis, in_regs, force, order in combos(A):
            got = built(A, i, dt, V_BASIS if vbasis else K_BASIS, in_regs, force, order)
            assert_same_bits(got, parent_loops(A, i, dt, vbasis, in_regs, force, order), (name, i, dt, vbasis, in_regs, force, order))
            ncases += 1
        assert ncases == len(A) * len(DTS) * (16 if vbasis_possible(A) else 8)


def test_structure_of_the_stage_terms():
    for name in METHODS:
        check_structure(name, tableau(name))


def check_structure(name, A):
    ns = len(A)
    for i, dt, vbasis, in_regs, force, order in combos(A):
        what = (name, i, dt, vbasis, in_regs, force, order)
        got = built(A, i, dt, V_BASIS if vbasis else K_BASIS, in_regs, force, order)
        stage_terms = [(s, c) for s, c in got["terms"] if s < ns]
        assert len(got["terms"]) <= MAX_STAGES + 1, what
        assert all(0 <= s < i for s, _ in stage_terms) and [s for s, _ in stage_terms] == sorted({s for s, _ in stage_terms}), what
        assert all(c != 0.0 for _, c in stage_terms), what
        assert (len(got["terms"]) - len(stage_terms)) == int(force) and (not force or got["terms"][-1][0] == ns), what
        later = any(A[i2, i] != 0.0 for i2 in range(i + 1, ns))
        assert got["write_k"] == int(later and not vbasis), what
        if vbasis:
            beta = dict(stage_terms)
            if got["self_in"] != 0.0:
                assert in_regs and i - 1 not in beta, what
                beta[i - 1] = got["self_in"]
            if not in_regs:
                assert got["self_in"] == 0.0, what
            c0m1 = 0.0
            for m in sorted(beta):  # minus the sum of every non-zero β in index order, the one that went to self_in included
                c0m1 -= beta[m]
            assert bits(got["c0m1"]) == bits(c0m1), what
            # no β contains Δt
            other = built(A, i, 7.0 * dt, V_BASIS, in_regs, force, order)
            assert [(s, bits(c)) for s, c in other["terms"] if s < ns] == [(s, bits(c)) for s, c in stage_terms], what
            assert bits(other["c0m1"]) == bits(got["c0m1"]) and bits(other["self_in"]) == bits(got["self_in"]), what
        else:
            assert got["c0m1"] == 0.0 and got["self_in"] == 0.0, what


def test_rk44_stage_velocity_weights_known_answer():
    """β_3 = (1/3, 2/3, 1/3), every other β zero; each is one division of exactly represented or once-rounded inputs: 2 ulp."""
    A = tableau("RK44")
    want = {0: {}, 1: {}, 2: {}, 3: {0: 1 / 3, 1: 2 / 3, 2: 1 / 3}}
    for i in range(4):
        for in_regs in (False, True):
            got = built(A, i, 1e-3, V_BASIS, in_regs)
            beta = dict(got["terms"])
            if got["self_in"] != 0.0:
                beta[i - 1] = got["self_in"]
            assert set(beta) == set(want[i])
            for m, b in want[i].items():
                assert abs(beta[m] - b) <= 2 * math.ulp(b)
            assert (got["self_in"] != 0.0) == (in_regs and i == 3)
            assert abs(got["c0m1"] + sum(want[i].values())) <= 4 * math.ulp(4 / 3)


def test_reference_order_list_is_the_parent_loops_bit_for_bit():
    """Σ_{j<=i} Δt A[i,j] k_j of the loops that run the reference's kernel sequence: products in double (rk_step_any, ins_rk_step_ext_f64) and, on the
    Float32 path, Δt (float)A[i,j] in float (rk32_step); the force coefficient adds every product in index order before the zero skip."""
    for name, dt, force in itertools.product(METHODS, DTS, (False, True)):
        A = tableau(name)
        check_reference_order(name, A, dt, force)


def check_reference_order(name, A, dt, force):
    ns = len(A)
    for i in range(ns):
        for kind, S in ((SUM_F64, np.float64), (SUM_F32, np.float32)):
            terms, cf = [], S(0)
            for j in range(i + 1):
                c = S(dt) * S(A[i, j])
                cf = cf + c
                if c == 0:
                    continue
                terms.append((j, float(c)))
            if force:
                terms.append((ns, float(cf)))
            got = built(A, i, dt, kind, force=force)
            assert [(s, bits(c)) for s, c in got["terms"]] == [(s, bits(c)) for s, c in terms], (name, i, dt, force, kind)
            assert bits(got["cforce"]) == bits(float(cf) if force else 0.0), (name, i, dt, force, kind)
