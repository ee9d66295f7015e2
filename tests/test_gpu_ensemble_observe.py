"""Observing an ensemble (`ensemble_stats`, `get_cfl_timestep_ensemble`, `observespectrum_ensemble`, `solve_unsteady_ensemble`;
csrc/ins_rk_ensemble_observe.hip) against the per-member observers and the CPU oracle, on the boxes of tests/test_gpu_ensemble.py:
  16 x 32   the one-launch solve, smallest side, one 64-column tile of the statistics kernel with 48 idle lanes,
  64 x 64   two x tiles of the stage kernel, a full tile of the statistics kernel, four row chunks,
  128 x 16  the three-pass solve layout, two column tiles, one row chunk.
Members: `random_field` with different seeds (solenoidal: max|div u| at rounding level), one field that is not solenoidal (max|div u| of order |u|/Δ, so
that a relative comparison with the oracle means something), one all-zero member.  B = 1, 3, 7 are the first members of that list."""
import numpy as np
import pytest
import torch

from tests import fixtures as fx
from tests.test_gpu_parity import relmax

pytestmark = pytest.mark.gpu

GRIDS = [(16, 32), (64, 64), (128, 16)]
BS = (1, 3, 7)
OP_TOL = 1e-12  # tests/test_gpu_fields.py: a single operator against the oracle


@pytest.fixture(scope="module")
def ins():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


_CASES = {}


def _case(ins, o, n):
    """Setup, solver, the seven members (ghosts valid) and their per-member references, built once per box and left unchanged."""
    if n in _CASES:
        return _CASES[n]
    x = tuple(np.linspace(0.0, 1.0, ni + 1) for ni in n)
    sp = ins.Setup(x=x, Re=500.0, device="cuda:0")
    ps = ins.psolver_spectral(sp)
    so = o.make_setup(x, Re=500.0)
    rough = ins.apply_bc_u_(ins.from_numpy(sp, 0.3 * fx.randn_field(sp.grid.N + (2,), 5)), 0.0, sp)
    rf = [ins.apply_bc_u_(ins.random_field(sp, 0.0, kp=4, psolver=ps, seed=50 + b), 0.0, sp) for b in range(5)]
    members = [rf[0], torch.zeros_like(rf[0]), rough] + rf[1:]
    ref = dict(E=[ins.total_kinetic_energy(u, sp) for u in members], maxdiv=[ins.max_abs_divergence(u, sp) for u in members],
               cfl=[ins.get_cfl_timestep_(None, u, sp) for u in members],
               ehat=[ins.observespectrum(dict(u=u, temp=None, t=0.0, n=0), setup=sp)["ehat"].value.copy() for u in members])
    _CASES[n] = (sp, ps, so, members, ref)
    return _CASES[n]


def _padded(sp, members, pad=37, sentinel=-7.25):
    """The members in one buffer with `pad` sentinel elements in front of every member: a member stride beyond a vector field."""
    B, nvec = len(members), int(np.prod(sp.grid.N)) * 2
    stride = nvec + pad
    buf = torch.full((pad + B * stride,), sentinel, dtype=torch.float64, device=sp.device)
    N0, N1 = sp.grid.N
    U = buf[pad:].as_strided((B, N0, N1, 2), (stride, 1, N0, N0 * N1))
    for b, u in enumerate(members):
        U[b].copy_(u)
    return buf, U


@pytest.mark.parametrize("n", GRIDS)
def test_stats_match_per_member_observers_and_oracle(ins, oracle, n):
    o = oracle
    sp, ps, so, members, ref = _case(ins, o, n)
    ncell = n[0] * n[1]
    sl = tuple(slice(lo, hi) for lo, hi in so.grid.Ip)
    for B in BS:
        cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)
        buf, U = _padded(sp, members[:B])
        before = buf.clone()
        st = ins.ensemble_stats(cache, U)
        assert set(st) == {"E", "maxdiv", "Δt_cfl"} and all(v.shape == (B,) and v.dtype == torch.float64 and v.is_cuda for v in st.values())
        E, maxdiv, cfl = (st[k].cpu().numpy().copy() for k in ("E", "maxdiv", "Δt_cfl"))
        assert torch.equal(buf, before)  # U unchanged, padding untouched
        for b in range(B):
            print(n, B, b, "E", E[b], ref["E"][b], "maxdiv", maxdiv[b], ref["maxdiv"][b], "cfl", cfl[b], ref["cfl"][b])
            assert maxdiv[b] == ref["maxdiv"][b] and cfl[b] == ref["cfl"][b]  # max and min are exact: bitwise
            assert abs(E[b] - ref["E"][b]) <= 2 * ncell * 2.0**-53 * ref["E"][b]  # non-negative terms summed in another order, on both sides
            # the oracle, at the single-operator tolerance.  The divergence is a difference of terms of size |u| / Δ: its error is relative to those
            u_h = ins.to_numpy(members[b])
            assert abs(E[b] - o.total_kinetic_energy(u_h, so)) <= OP_TOL * max(o.total_kinetic_energy(u_h, so), 1e-300)
            assert abs(cfl[b] - o.get_cfl_timestep(u_h, so)) <= OP_TOL * o.get_cfl_timestep(u_h, so)
            size = np.max(np.abs(u_h)) * sum(ni for ni in n)
            assert abs(maxdiv[b] - np.max(np.abs(o.divergence(u_h, so)[sl]))) <= OP_TOL * max(size, 1e-300)
        assert ins.get_cfl_timestep_ensemble(cache, U) == min(ref["cfl"][:B])
        if B >= 3:  # the zero member: no energy, no divergence, the pure diffusive step
            assert E[1] == 0.0 and maxdiv[1] == 0.0 and cfl[1] == ins.get_cfl_timestep_(None, ins.vectorfield(sp), sp)
            assert relmax(np.array([maxdiv[2]]), np.array([np.max(np.abs(o.divergence(ins.to_numpy(members[2]), so)[sl]))])) < OP_TOL  # not solenoidal
    # permuting the members permutes the rows, bitwise (B = 7 from the loop)
    perm = [3, 0, 6, 1, 5, 2, 4]
    _, Uq = _padded(sp, [members[q] for q in perm])
    got = {k: v.cpu().numpy().copy() for k, v in ins.ensemble_stats(cache, Uq).items()}
    for b, q in enumerate(perm):
        assert got["E"][b] == E[q] and got["maxdiv"][b] == maxdiv[q] and got["Δt_cfl"][b] == cfl[q]


@pytest.mark.parametrize("n", GRIDS)
def test_spectrum_matches_per_member_observer_and_oracle(ins, oracle, n):
    o = oracle
    sp, ps, so, members, ref = _case(ins, o, n)
    rows = {}
    for B in BS:
        cache = ins.EnsembleCache(ins.RKMethods.RK44(), sp, ps, B)
        buf, U = _padded(sp, members[:B])
        before = buf.clone()
        out = ins.observespectrum_ensemble(cache, U)
        assert out["ehat"].shape == (B, len(out["κ"])) and torch.equal(buf, before)
        assert ins.observespectrum_ensemble(cache, U)["ehat"] is not out["ehat"] and len(cache._spectra) == 1  # the handle is cached, the result is a copy
        rows[B] = out["ehat"]
        for b in range(B):
            if b == 1:
                assert not out["ehat"][b].any()  # the zero member: exactly 0
                continue
            e_h, kap = o.observespectrum(ins.to_numpy(members[b]), so)
            assert np.array_equal(out["κ"], kap)
            print(n, B, b, relmax(out["ehat"][b], ref["ehat"][b]), relmax(out["ehat"][b], e_h))
            assert relmax(out["ehat"][b], ref["ehat"][b]) < 1e-12  # the hipFFT route of the single field
            assert relmax(out["ehat"][b], e_h) < 1e-12
    for B in BS[:-1]:  # a member's row does not depend on B
        assert np.array_equal(rows[B], rows[7][:B])


def _start(ins, sp, members, idx):
    U = ins.vectorfields(sp, len(idx))
    for b, q in enumerate(idx):
        U[b].copy_(members[q])
    return U


@pytest.mark.parametrize("n", [(16, 32), (128, 16)])  # one box per solve route
def test_adaptive_driver_is_solve_unsteady_per_member(ins, oracle, n):
    sp, ps, so, members, ref = _case(ins, oracle, n)
    method = ins.RKMethods.RK44()
    dt0 = 0.9 * ref["cfl"][0]
    tlims = (0.0, 5.6 * dt0)  # about six steps, the last one clipped
    (u1, _, t1), out = ins.solve_unsteady(setup=sp, tlims=tlims, ustart=members[0], psolver=ps, method=method, Δt=None,
                                          processors=dict(log=ins.processor(lambda s: _record(s))))
    want_ts = out["log"]
    got_ts = []
    (U, t), dts = ins.solve_unsteady_ensemble(cache=ins.EnsembleCache(method, sp, ps, 1), U=_start(ins, sp, members, [0]), tlims=tlims, Δt=None,
                                              observe=lambda V, t, k: got_ts.append(t))
    assert 5 <= len(dts) <= 8 and got_ts == want_ts and t == t1 and torch.equal(U[0], u1)  # the same times: the same Δt at every step
    assert dts[0] == dt0
    # B = 3: one Δt for all, the smallest of the members' CFL steps; every member is timestep_ replayed with the recorded list
    idx = [0, 3, 4]
    cache = ins.EnsembleCache(method, sp, ps, 3)
    U0 = _start(ins, sp, members, idx)
    seen = []
    (U, t), dts = ins.solve_unsteady_ensemble(cache=cache, U=U0, tlims=tlims, Δt=None, observe=lambda V, t, k: seen.append((k, t, V.clone())))
    assert [k for k, _, _ in seen] == list(range(len(dts) + 1)) and U is not U0 and torch.equal(U0[1], members[3]) and t == pytest.approx(tlims[1], rel=1e-14)
    for (k, _, V), dt in zip(seen, dts):
        percfl = [ins.get_cfl_timestep_(None, V[b], sp) for b in range(3)]
        assert dt == 0.9 * min(percfl) or k == len(dts) - 1  # the last step is clipped to tend
    for b, q in enumerate(idx):
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=ins.copyfield(members[q]))
        ec = ins.ode_method_cache(method, sp, ps)
        for dt in dts:
            st = ins.timestep_(method, st, dt, cache=ec)
        assert torch.equal(U[b], st.u), (n, b)
    # n_adapt_Δt = 4: batches of four steps in one native call are the same Δt list replayed step by step
    (U4, t4), dts4 = ins.solve_unsteady_ensemble(cache=cache, U=U0, tlims=tlims, Δt=None, n_adapt_Δt=4)
    assert len(set(dts4[:4])) == 1 and dts4[0] == dts[0] and t4 == pytest.approx(tlims[1], rel=1e-14)
    V = _start(ins, sp, members, idx)
    tt = 0.0
    for dt in dts4:
        ins.timesteps_ensemble_(cache, V, tt, dt, 1)
        tt += dt
    assert torch.equal(U4, V)


def _record(state):
    """processor: the times the states of a solve_unsteady run arrive with, the start included"""
    ts = [state.value["t"]]
    state.on(lambda s: ts.append(s["t"]))
    return ts


def test_fixed_step_driver_batches_between_observations(ins, oracle):
    n = (64, 64)
    sp, ps, so, members, ref = _case(ins, oracle, n)
    method = ins.RKMethods.RK44()
    dt = 0.5 * min(ref["cfl"][q] for q in (0, 3, 4))
    tlims = (0.0, 7 * dt)
    cache = ins.EnsembleCache(method, sp, ps, 3)
    seen = []
    (U, t), dts = ins.solve_unsteady_ensemble(cache=cache, U=_start(ins, sp, members, [0, 3, 4]), tlims=tlims, Δt=dt, nupdate=3,
                                              observe=lambda V, t, k: seen.append((k, t)))
    assert [k for k, _ in seen] == [0, 3, 6] and len(dts) == 7 and len(set(dts)) == 1
    # the call pattern of solve_unsteady with a processor of nupdate = 3: calls of 3, 3 and 1 steps, t accumulated the same way
    st, out = ins.solve_unsteady(setup=sp, tlims=tlims, ustart=members[3], psolver=ps, method=method, Δt=dt,
                                 processors=dict(p=ins.processor(lambda s: None, nupdate=3)))
    assert torch.equal(U[1], st[0]) and t == st[2]
    V = _start(ins, sp, members, [0, 3, 4])
    tt = 0.0
    for k in (3, 3, 1):
        ins.timesteps_ensemble_(cache, V, tt, dts[0], k)
        tt += k * dts[0]
    assert torch.equal(U, V)
    assert [tk for _, tk in seen][1] == 0.0 + 3 * 1.0 * dts[0]
