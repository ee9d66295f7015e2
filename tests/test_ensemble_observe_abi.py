"""CPU-side checks of the ensemble observers (csrc/ins_rk_ensemble_observe.hip; `ensemble_stats`, `get_cfl_timestep_ensemble`, `observespectrum_ensemble`,
`solve_unsteady_ensemble`): the entries are in include/ins_hip.h, exported and bound with the header's argument lists; the host-side checks of the wrappers
come before any native call; the control flow of the driver against stand-ins for the step and the CFL call; and the index re-addressing of the member
spectrum, restated in numpy, against the oracle's shells."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_ensemble_abi import _cache, _members

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ins_rk_ensemble_stats_f64", "ins_rk_ensemble_spectrum_create", "ins_rk_ensemble_spectrum_f64", "ins_rk_ensemble_spectrum_destroy"]


def _header_args(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ins_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in ins_hip.h"
    out = []
    for arg in m.group(1).split(","):
        arg = " ".join(arg.split())
        if arg.count("*") == 2:
            out.append("handle**")
        elif "int64_t*" in arg:
            out.append("int64*")
        elif "*" in arg:
            out.append("void*")
        else:
            out.append(arg.rsplit(" ", 1)[0])
    return out


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    vp = C.c_void_p
    ctype = {"void*": vp, "int64*": C.POINTER(C.c_int64), "handle**": C.POINTER(vp), "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [ctype[a] for a in _header_args(n)], (n, _header_args(n))
    assert _header_args("ins_rk_ensemble_stats_f64") == ["void*", "double", "void*", "int64_t", "void*", "void*"]
    assert _header_args("ins_rk_ensemble_spectrum_create") == ["void*", "int", "int64*", "int64*", "handle**"]
    assert _header_args("ins_rk_ensemble_spectrum_f64") == ["void*", "void*", "int64_t", "void*", "void*"]
    for f in ("ensemble_stats", "get_cfl_timestep_ensemble", "observespectrum_ensemble", "solve_unsteady_ensemble"):
        assert callable(getattr(ins_amd, f)), f
    # null arguments need no device
    assert lib.ins_rk_ensemble_stats_f64(None, 1.0, None, 0, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_ensemble_spectrum_create(None, 1, None, None, None) == -1
    assert lib.ins_rk_ensemble_spectrum_f64(None, None, 0, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_ensemble_spectrum_destroy(None) == 0


def test_wrappers_check_the_field_before_any_native_call():
    """The checks of `timesteps_ensemble_`: every handle of the stand-in cache raises when it is touched."""
    import ins_amd as ins

    N, B = (18, 34), 3
    c = _cache(N, B)
    good = _members(B, N)
    calls = [lambda U, cache=c: ins.ensemble_stats(cache, U), lambda U, cache=c: ins.get_cfl_timestep_ensemble(cache, U),
             lambda U, cache=c: ins.observespectrum_ensemble(cache, U),
             lambda U, cache=c: ins.solve_unsteady_ensemble(cache=cache, U=U, tlims=(0.0, 1.0), Δt=0.1)]
    for call in calls:
        with pytest.raises(TypeError, match="float64"):  # wrong dtype
            call(_members(B, N, torch.float32))
        for bad in (good[0], _members(B, (18, 18)), good[..., 0]):  # wrong shape
            with pytest.raises(ValueError, match="shape"):
                call(bad)
        with pytest.raises(ValueError, match="B = 3"):  # wrong B
            call(_members(B + 1, N))
        with pytest.raises(ValueError, match="overlap"):  # overlapping members
            call(good[:1].expand(B, -1, -1, -1))
        with pytest.raises(TypeError, match="EnsembleCache"):  # not an EnsembleCache
            call(good, cache=SimpleNamespace())


class _FakeRun:
    """Stand-ins for `timesteps_ensemble_` and `get_cfl_timestep_ensemble` inside solver.py: record the calls, hand out CFL steps from a list."""

    def __init__(self, monkeypatch, cfls):
        from ins_amd import solver

        self.steps, self.cfl_calls, self.cfls = [], 0, list(cfls)
        monkeypatch.setattr(solver, "_ensemble_ustride", lambda cache, U: 0)
        monkeypatch.setattr(solver, "timesteps_ensemble_", lambda cache, U, t, dt, k: self.steps.append((t, dt, k)))
        monkeypatch.setattr(solver, "get_cfl_timestep_ensemble", self._cfl)
        self.cache = SimpleNamespace(method=SimpleNamespace(c=[0.5, 0.5, 1.0]), B=2)

    def _cfl(self, cache, U):
        self.cfl_calls += 1
        return self.cfls[min(self.cfl_calls, len(self.cfls)) - 1]

    def run(self, **kw):
        import ins_amd as ins

        return ins.solve_unsteady_ensemble(cache=self.cache, U="U", docopy=False, **kw)


def test_driver_adaptive_clips_to_tend_and_honours_the_floor(monkeypatch):
    f = _FakeRun(monkeypatch, [0.4, 0.2, 0.01, 0.4])
    (U, t), dts = f.run(tlims=(0.0, 1.0), cfl=0.5, Δt_min=0.05)
    # 0.5·0.4, 0.5·0.2, the floor 0.05 instead of 0.005, then 0.2 until the last step is clipped
    assert U == "U" and dts[:3] == [0.2, 0.1, 0.05] and all(d == 0.2 for d in dts[3:-1]) and t == pytest.approx(1.0, rel=1e-15)
    assert dts[-1] == pytest.approx(1.0 - sum(dts[:-1]), rel=1e-12) and 0 < dts[-1] <= 0.2
    assert all(k == 1 for _, _, k in f.steps) and f.cfl_calls == len(dts)  # n_adapt_Δt = 1: one CFL read and one native call per step
    ts = [0.0]
    for d in dts[:-1]:
        ts.append(ts[-1] + 1.0 * d)  # timestep_: t + c[-1] Δt
    assert [s[0] for s in f.steps] == ts


def test_driver_batches_adaptive_steps_only_when_they_fit(monkeypatch):
    f = _FakeRun(monkeypatch, [0.2])
    (U, t), dts = f.run(tlims=(0.0, 1.1), cfl=0.5, n_adapt_Δt=4)
    # Δt = 0.1: 4 + 4 steps fit before 1.1 and run as one call each; of the third four only three are left: step by step, the last one clipped
    assert [k for _, _, k in f.steps] == [4, 4, 1, 1, 1] and f.cfl_calls == 3 and len(dts) == 11
    assert dts[:10] == [0.1] * 10 and dts[10] == pytest.approx(0.1, rel=1e-12) and t == pytest.approx(1.1, rel=1e-15)
    assert f.steps[1][0] == 0.0 + 4 * 1.0 * 0.1  # the time of a batch, as timesteps_ forms it
    # with an observer the batches also stop at the multiples of nupdate
    f = _FakeRun(monkeypatch, [0.2])
    seen = []
    f.run(tlims=(0.0, 1.1), cfl=0.5, n_adapt_Δt=4, nupdate=3, observe=lambda U, t, n: seen.append(n))
    assert seen == [0, 3, 6, 9] and [k for _, _, k in f.steps][:5] == [3, 1, 2, 2, 1]


def test_driver_fixed_step_schedule(monkeypatch):
    f = _FakeRun(monkeypatch, [])
    seen = []
    (U, t), dts = f.run(tlims=(0.0, 0.7), Δt=0.1000001, nupdate=3, observe=lambda U, t, n: seen.append((n, t)))
    assert f.cfl_calls == 0 and [k for _, _, k in f.steps] == [3, 3, 1] and len(dts) == 7 and len(set(dts)) == 1 and dts[0] == 0.7 / 7
    assert [n for n, _ in seen] == [0, 3, 6] and seen[1][1] == 0.0 + 3 * 1.0 * dts[0]
    f = _FakeRun(monkeypatch, [])
    (U, t), dts = f.run(tlims=(0.0, 0.7), Δt=0.1)  # nobody looks: the whole loop is one native call
    assert [k for _, _, k in f.steps] == [7]
    with pytest.raises(ValueError, match="positive"):
        f.run(tlims=(0.0, 0.7), Δt=0.1, nupdate=0)


@pytest.mark.parametrize("n", [(16, 32), (64, 64), (128, 16)])
def test_member_spectrum_readdressing_against_the_oracle_shells(oracle, n):
    """Gathering with the re-addressed positions from a spectrum stored as the library's passes leave it gives what the oracle's shells give on the K-array."""
    from ins_amd.processors import _member_spectrum_positions, _yfft_storage_position

    o = oracle
    so = o.make_setup(tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n), Re=100.0)
    inds, κ, K = o.spectral_stuff(so)
    assert K == (n[0] // 2, n[1] // 2)
    pos_of = _yfft_storage_position(n[1])
    assert sorted(pos_of) == list(range(n[1])) and pos_of[0] == 0  # a permutation that keeps the mean mode in place
    nb, kxs = 3, (n[0] // 2 + 1 + 7) // 8 * 8
    rs = 2 * nb * kxs
    rng = np.random.default_rng(0)
    full = rng.standard_normal((n[0] // 2 + 1, n[1]))  # one line set in natural order: (kx, ky)
    stored = np.zeros(rs * n[1])
    line = 2 * 1 + 1  # member 1, component 1
    for ky in range(n[1]):
        stored[line * kxs + rs * pos_of[ky]: line * kxs + rs * pos_of[ky] + full.shape[0]] = full[:, ky]
    Karr = full[: K[0], : K[1]].reshape(-1, order="F")
    for shell in inds:
        p = _member_spectrum_positions(n, shell, rs, pos_of)
        assert np.array_equal(stored[line * kxs + p], Karr[shell])
