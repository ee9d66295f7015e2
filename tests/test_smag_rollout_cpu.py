"""CPU-side checks of the Smagorinsky closure in the native reverse loop: the four new symbols are exported and bound with the header's
signatures, and the θ bookkeeping of `_autodiff_core.timesteps` / `_TimeSteps` / `_StepAdjoint` / `_SmagorinskyForce` on the stand-in table of
tests/test_autodiff_core_cpu.py, with a torch Smagorinsky stand-in m(u, θ) = θ² u·roll(u, 1, 0) for the two new table entries.

What the bookkeeping test pins: θ reaches every recomputation (forward chunks and the step-start states of the backward), θbar is zeroed once per
backward and summed over all steps and chunks (one tensor is handed to the handle, once), and the handle's closure is cleared afterwards.
Tolerance: 1e-12 relative in float64, as in tests/test_autodiff_core_cpu.py (the same arithmetic in another association order at most)."""
import ctypes as C

import pytest
import torch

from tests.test_ad_rollout_abi import _header_args
from tests.test_autodiff_core_cpu import SHAPES, close, make, plain_step, rand

NAMES = ["ins_smagorinsky_force_pullback_f64", "ins_smagorinsky_force_pullback_f32", "ins_rk_adjoint_set_closure", "ins_rk_adjoint_set_closure_f32"]


def test_symbols_exported_and_bound():
    import ins_amd

    lib = ins_amd._lib.load()
    vp = C.c_void_p
    ctype = {"void*": vp, "int": C.c_int, "int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [ctype[a] for a in _header_args(n)], (n, _header_args(n))
    assert len(ins_amd._lib.SIGNATURES["ins_smagorinsky_force_pullback_f64"][1]) == 8
    assert callable(ins_amd.ad.smagorinsky_force) and callable(ins_amd.ad32.smagorinsky_force)


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    assert lib.ins_smagorinsky_force_pullback_f64(None, 0.1, None, None, None, 0, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_smagorinsky_force_pullback_f32(None, 0.1, None, None, None, 0, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_set_closure(None, 1, 0.1, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_set_closure_f32(None, 1, 0.1, None) == -1 and b"null" in lib.ins_last_error()


# ------------------------------------------------------------------------------------ the stand-in closure and the stand-in native entries
def m_plain(u, θ):
    return θ * θ * u * torch.roll(u, 1, 0)


def table(core, dtype, with_temp, D=2):
    """(setup, ops, log): the stand-in table with the two closure entries and stand-in "native" rollout entries that log their calls."""
    import ins_amd as ins

    setup, ops = make(D, dtype, with_temp)
    log = []

    def force_(s, u, θ, sp):
        assert isinstance(θ, float)
        return s.copy_(m_plain(u, θ))

    def force_pullback_(ubar, θbar, sbar, u, θ, sp):
        ubar.copy_(θ * θ * (sbar * torch.roll(u, 1, 0) + torch.roll(sbar * u, -1, 0)))
        if θbar is not None:
            assert θbar.dtype == torch.float64 and θbar.dim() == 0
            θbar.add_(2 * θ * (sbar * u * torch.roll(u, 1, 0)).sum().double())
        return ubar, θbar

    def step(adj, u, temp, Δt, θ):
        return core.timestep(ops, adj.erk, ins.create_stepper(adj.erk, setup=setup, psolver=None, u=u, temp=temp), Δt, θ)

    def rk_steps_(adj, u, temp, t, Δt, nsteps, θ=None):
        log.append(("steps", nsteps, θ))
        with torch.no_grad():
            for _ in range(nsteps):
                st = step(adj, u, temp, Δt, θ)
                u.copy_(st.u)
                if temp is not None:
                    temp.copy_(st.temp)

    def rk_adjoint_set_closure(adj, θ, θbar):
        log.append(("set_closure", θ, None if θbar is None else id(θbar), None if θbar is None else float(θbar)))
        adj.state = (θ, θbar)

    def rk_step_pullback_(adj, ubar, tempbar, ustart, tempstart, Δt):
        θ, θbar = getattr(adj, "state", (None, None))
        log.append(("pullback", θ))
        with torch.enable_grad():
            xs = [ustart.detach().clone().requires_grad_(True)] + ([] if tempstart is None else [tempstart.detach().clone().requires_grad_(True)])
            th = None if θ is None else torch.tensor(θ, dtype=dtype, requires_grad=True)
            st = step(adj, xs[0], None if tempstart is None else xs[1], Δt, th)
            outs, bars = [st.u] + ([] if tempstart is None else [st.temp]), [ubar.clone()] + ([] if tempstart is None else [tempbar.clone()])
            gs = torch.autograd.grad(outs, xs + ([] if th is None else [th]), bars)
        ubar.copy_(gs[0])
        if tempbar is not None:
            tempbar.copy_(gs[1])
        if θbar is not None:
            θbar.add_(gs[-1].double())

    ops.check_closure_inputs = lambda sp, u, *others: None
    ops.smagorinsky_force_, ops.smagorinsky_force_pullback_ = force_, force_pullback_
    ops.rk_cache = lambda erk, sp, ps: None
    ops.rk_adjoint_create = lambda erk, sp, ps: object()
    ops.rk_adjoint_destroy = lambda h: None
    ops.rk_steps_, ops.rk_step_pullback_, ops.rk_adjoint_set_closure = rk_steps_, rk_step_pullback_, rk_adjoint_set_closure
    ops.rk_copy_ = lambda dst, src, sp, vector: dst.copy_(src)
    setup.closure_model = lambda u, θ: core.smagorinsky_force(ops, u, θ, setup)
    return setup, ops, log


@pytest.mark.parametrize("with_temp", [False, True])
@pytest.mark.parametrize("nsteps,every", [(1, 1), (5, 1), (5, 2), (5, 5)])
def test_timesteps_with_theta_matches_unrolled_autograd(nsteps, every, with_temp):
    import ins_amd as ins

    core = ins._autodiff_core
    dtype, D, Δt = torch.float64, 2, 0.05
    setup, ops, log = table(core, dtype, with_temp)
    meth = ins.RKMethods.RK44()
    N = SHAPES[D]
    w, wt = rand(N + (D,), dtype, 3), rand(N, dtype, 4)
    adj = core._StepAdjoint(ops, meth, setup, None)
    out = []
    for route in ("rollout", "unrolled"):
        u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
        t0 = rand(N, dtype, 2).requires_grad_(True) if with_temp else None
        θ = torch.tensor(0.4, dtype=dtype, requires_grad=True)
        if route == "rollout":
            st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=u0, temp=t0), Δt, nsteps, every, adj=adj, θ=θ)
            u, temp = st.u, st.temp
            assert st.n == nsteps
        else:
            plain = type(setup)(**{**vars(setup), "closure_model": m_plain})
            u, temp = u0, t0
            for _ in range(nsteps):
                u, temp = plain_step(meth, plain, u, temp, Δt, θ)
        loss = (u * u * w).sum() + (0 if temp is None else (temp * temp * wt).sum())
        loss.backward()
        out.append([x for x in (u.detach(), u0.grad, None if t0 is None else t0.grad, θ.grad.reshape(1)) if x is not None])
    for a, b in zip(*out):
        assert a.dtype == dtype and close(a, b, dtype)
    # θ reaches every recomputation; θbar: one zeroed tensor handed over once per backward; the closure is cleared afterwards
    chunks = [min(every, nsteps - s) for s in range(0, nsteps, every)]
    expect = [("steps", n, 0.4) for n in chunks]
    sets = [e for e in log if e[0] == "set_closure"]
    assert len(sets) == 2 and sets[0][1] == 0.4 and sets[0][3] == 0.0 and sets[1][1:] == (None, None, None)
    for n in reversed(chunks):
        expect += [("steps", 1, 0.4)] * (n - 1) + [("pullback", 0.4)] * n
    assert [e for e in log if e[0] != "set_closure"] == expect
    assert log.index(sets[0]) == len(chunks) and log[-1] == sets[1] and not adj.closure_on


def test_handle_serves_calls_with_and_without_theta():
    """One `_StepAdjoint`: a rollout with θ, then one without (closure_model removed): the second runs as if the first had never happened."""
    import ins_amd as ins

    core = ins._autodiff_core
    dtype, D = torch.float64, 2
    setup, ops, log = table(core, dtype, False)
    meth = ins.RKMethods.RK44()
    N = SHAPES[D]
    w = rand(N + (D,), dtype, 3)
    adj = core._StepAdjoint(ops, meth, setup, None)

    def run(θ):
        u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
        st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=u0), 0.05, 3, 2, adj=adj, θ=θ)
        (st.u * st.u * w).sum().backward()
        return u0.grad

    model = setup.closure_model
    setup.closure_model = None
    before = run(None)
    setup.closure_model = model
    run(torch.tensor(0.4, dtype=dtype, requires_grad=True))
    setup.closure_model = None
    del log[:]
    after = run(None)
    assert torch.equal(before, after)
    assert all(e[0] != "set_closure" for e in log) and all(e[-1] is None for e in log)


def test_float_theta_gives_no_theta_gradient_and_the_same_field_gradient():
    import ins_amd as ins

    core = ins._autodiff_core
    dtype, D = torch.float64, 2
    setup, ops, log = table(core, dtype, False)
    meth = ins.RKMethods.RK44()
    N = SHAPES[D]
    w = rand(N + (D,), dtype, 3)
    adj = core._StepAdjoint(ops, meth, setup, None)
    grads = []
    for θ in (torch.tensor(0.4, dtype=dtype, requires_grad=True), 0.4):
        u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
        st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=u0), 0.05, 3, 2, adj=adj, θ=θ)
        (st.u * st.u * w).sum().backward()
        grads.append(u0.grad)
    assert torch.equal(*grads)
    sets = [e for e in log if e[0] == "set_closure" and e[1] is not None]
    assert len(sets) == 2 and sets[0][2] is not None and sets[1][2] is None  # no θ cotangent is asked of the handle for a float θ
    # only θ requires grad: the same number
    θ = torch.tensor(0.4, dtype=dtype, requires_grad=True)
    st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=rand(N + (D,), dtype, 1)), 0.05, 3, 2, adj=adj, θ=θ)
    (st.u * st.u * w).sum().backward()
    θ2 = torch.tensor(0.4, dtype=dtype, requires_grad=True)
    u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
    st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=u0), 0.05, 3, 2, adj=adj, θ=θ2)
    (st.u * st.u * w).sum().backward()
    assert torch.equal(θ.grad, θ2.grad) and float(θ.grad) != 0.0


@pytest.mark.parametrize("which", ["ad", "ad32"])
def test_refusals_without_gpu(which):
    """Every closure that is not the library's Smagorinsky closure of this setup with θ keeps raising the present NotImplementedError."""
    import ins_amd as ins
    from tests.test_ad_rollout_abi import _ps32, _setup, _stepper
    from types import SimpleNamespace

    ad = getattr(ins, which)
    mine = torch.float64 if which == "ad" else torch.float32
    ps = SimpleNamespace() if which == "ad" else _ps32()
    method = ins.RKMethods.RK44()

    def tagged(sp, name=which):
        def closure(u, θ):
            return u
        closure._ad_smagorinsky = (name, sp)
        return closure

    other = _setup()
    cases = []
    sp = _setup(closure_model=lambda u, θ: u)
    cases.append((sp, 0.17))  # a lambda closure
    sp = _setup()
    sp.closure_model = tagged(sp)
    cases.append((sp, None))  # the Smagorinsky closure without θ
    cases.append((_setup(), 0.17))  # θ without a closure
    sp = _setup()
    sp.closure_model = tagged(other)
    cases.append((sp, 0.17))  # a Smagorinsky closure built for another setup
    sp = _setup()
    sp.closure_model = tagged(sp, "ad32" if which == "ad" else "ad")
    cases.append((sp, 0.17))  # the other precision's closure
    for sp, θ in cases:
        with pytest.raises(NotImplementedError, match="timestep "):
            ad.timesteps(method, _stepper(sp, ps, mine), 1e-3, 2, θ=θ)
