"""CPU-side checks of the generic native reverse step (csrc/ins_rk_adjoint_loop.h: ins_rk_step_pullback_f32, ins_rk_step_pullback_ext_f64 / _f32) and of
`ad.timesteps` / `ad32.timesteps`: the symbols are exported and bound with the header's signatures, the refusals that need no device, and the checkpoint
and chunk bookkeeping of `_autodiff_core._TimeSteps` for the pair state (u, temp) on the stand-in operators of tests/test_autodiff_core_cpu.py."""
import ctypes as C
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests.test_autodiff_core_cpu import SHAPES, close, make, rand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ins_rk_adjoint_create_f32", "ins_rk_adjoint_destroy_f32", "ins_rk_step_pullback_f32", "ins_rk_adjoint_set_temperature",
         "ins_rk_adjoint_set_temperature_f32", "ins_rk_step_pullback_ext_f64", "ins_rk_step_pullback_ext_f32"]


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
    ctype = {"void*": vp, "double*": dp, "handle**": C.POINTER(vp), "int": C.c_int, "double": C.c_double, "float": C.c_float}
    for n in NAMES:
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ins_amd._lib.SIGNATURES, f"{n} is not bound"
        res, args = ins_amd._lib.SIGNATURES[n]
        assert res is C.c_int and getattr(lib, n).argtypes == args
        assert args == [ctype[a] for a in _header_args(n)], (n, _header_args(n))
    assert callable(ins_amd.ad32.timesteps) and callable(ins_amd.ad.timesteps)


def test_null_arguments_without_gpu():
    import ins_amd

    lib = ins_amd._lib.load()
    assert lib.ins_rk_adjoint_create_f32(None, None, 4, None, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_step_pullback_f32(None, 1e-3, None, None, 1e-3, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_step_pullback_ext_f64(None, 1e-3, None, None, None, 1e-3, None, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_step_pullback_ext_f32(None, 1e-3, None, None, None, 1e-3, None, None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_set_temperature(None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_set_temperature_f32(None, None) == -1 and b"null" in lib.ins_last_error()
    assert lib.ins_rk_adjoint_destroy_f32(None) == 0


# ------------------------------------------------------------------------------------ refusals of the public functions
def _stepper(setup, psolver, udtype, tdtype=None, N=(4, 4)):
    temp = None if tdtype is None else torch.zeros(N, dtype=tdtype)
    return SimpleNamespace(setup=setup, psolver=psolver, u=torch.zeros(N + (len(N),), dtype=udtype), temp=temp, t=0.0, n=0)


def _setup(**kw):
    """A stand-in setup: nothing here reaches the device, every refusal comes first."""
    d = dict(temperature=None, closure_model=None, bodyforce=None, issteadybodyforce=False, needs_bc_planes=False, boundary_conditions=(),
             grid=SimpleNamespace(N=(4, 4), dimension=2), device=torch.device("cpu"))
    d.update(kw)
    return SimpleNamespace(**d)


def _ps32():
    import ins_amd

    return object.__new__(ins_amd.f32.psolver_spectral32)


@pytest.mark.parametrize("which", ["ad", "ad32"])
def test_refusals_without_gpu(which):
    import ins_amd as ins
    from ins_amd.boundary_conditions import DirichletBC, HaloBC

    ad = getattr(ins, which)
    mine, other = (torch.float64, torch.float32) if which == "ad" else (torch.float32, torch.float64)
    ps = SimpleNamespace() if which == "ad" else _ps32()
    wrong_ps = _ps32() if which == "ad" else SimpleNamespace()
    method = ins.RKMethods.RK44()
    step = ("ad.timestep " if which == "ad" else "timestep ")
    T = SimpleNamespace(boundary_conditions=((DirichletBC(1.0), DirichletBC(0.0)),) * 2)
    Tfun = SimpleNamespace(boundary_conditions=((DirichletBC(lambda x, y, t: 1.0 + 0 * x), DirichletBC(0.0)),) * 2)
    # ValueError: the counts, and a temperature field without an equation
    with pytest.raises(ValueError, match="nsteps"):
        ad.timesteps(method, _stepper(_setup(), ps, mine), 1e-3, 0)
    with pytest.raises(ValueError, match="checkpoint_every"):
        ad.timesteps(method, _stepper(_setup(), ps, mine), 1e-3, 3, checkpoint_every=0)
    with pytest.raises(ValueError, match="needs setup.temperature"):
        ad.timesteps(method, _stepper(_setup(), ps, mine, mine), 1e-3, 2)
    # TypeError: mixed precisions; the message for the other precision's field names the other module
    with pytest.raises(TypeError, match=r"ad32\.timesteps" if which == "ad" else r"ad\.timesteps"):
        ad.timesteps(method, _stepper(_setup(), ps, other), 1e-3, 2)
    with pytest.raises(TypeError, match="one precision"):
        ad.timesteps(method, _stepper(_setup(temperature=T), ps, mine, other), 1e-3, 2)
    with pytest.raises(TypeError, match="psolver"):
        ad.timesteps(method, _stepper(_setup(), wrong_ps, mine), 1e-3, 2)
    # NotImplementedError, each naming the step-by-step route
    refused = [
        (dict(closure_model=lambda u, θ: u), None),
        (dict(temperature=T), None),  # a temperature equation without stepper.temp
        (dict(needs_bc_planes=True), None),
        (dict(temperature=Tfun), mine),
        (dict(bodyforce=torch.zeros(4, 4, 2), issteadybodyforce=False), None),
        (dict(boundary_conditions=((HaloBC(), HaloBC()),)), None),
    ]
    for kw, tdtype in refused:
        with pytest.raises(NotImplementedError, match=step):
            ad.timesteps(method, _stepper(_setup(**kw), ps, mine, tdtype), 1e-3, 2)
    # two refused setups in one (the second's attributes over the first's; a temperature field where either has one).  Which reason is named is the
    # business of the shared list (core.check_rollout); the type is NotImplementedError, and a wrongly shaped field does not get in front of it
    for (a, ta), (b, tb) in itertools.combinations(refused, 2):
        for N in ((4, 4), (4, 5)):
            with pytest.raises(NotImplementedError):
                ad.timesteps(method, _stepper(_setup(**{**a, **b}), ps, mine, ta or tb, N=N), 1e-3, 2)


# ------------------------------------------------------------------------------------ checkpoint and chunk bookkeeping on the stand-in table
class StandInAdjoint:
    """`_StepAdjoint` on the stand-in table: the "native" step is `core.timestep` without grad, the "native" reverse step is torch's backward of
    one `core.timestep`, both in place like the native entries."""

    def __init__(self, core, ops, erk, setup):
        self.core, self.ops, self.erk, self.setup = core, ops, erk, setup
        self.log = []

    def _step(self, u, temp, Δt):
        import ins_amd as ins

        return self.core.timestep(self.ops, self.erk, ins.create_stepper(self.erk, setup=self.setup, psolver=None, u=u, temp=temp), Δt, None)

    def steps_(self, u, temp, t, Δt, nsteps):
        self.log.append(("steps", nsteps))
        with torch.no_grad():
            for _ in range(nsteps):
                st = self._step(u, temp, Δt)
                u.copy_(st.u)
                if temp is not None:
                    temp.copy_(st.temp)
        return u, temp

    def step_pullback_(self, ubar, ustart, Δt, tempbar=None, tempstart=None):
        self.log.append(("pullback",))
        with torch.enable_grad():
            xs = [ustart.detach().clone().requires_grad_(True)] + ([] if tempstart is None else [tempstart.detach().clone().requires_grad_(True)])
            st = self._step(xs[0], None if tempstart is None else xs[1], Δt)
            outs, bars = [st.u] + ([] if tempstart is None else [st.temp]), [ubar.clone()] + ([] if tempstart is None else [tempbar.clone()])
            gs = torch.autograd.grad(outs, xs, bars)
        ubar.copy_(gs[0])
        if tempbar is not None:
            tempbar.copy_(gs[1])


@pytest.mark.parametrize("with_temp", [False, True])
@pytest.mark.parametrize("every", [1, 2, 5])
@pytest.mark.parametrize("nsteps", [1, 5])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_timesteps_matches_chained_timestep(dtype, nsteps, every, with_temp):
    import ins_amd as ins

    core = ins._autodiff_core
    D = 2
    setup, ops = make(D, dtype, with_temp)
    ops.rk_copy_ = lambda dst, src, s, vector: dst.copy_(src)
    meth = ins.RKMethods.RK44()
    N = SHAPES[D]
    Δt = 0.05
    w, wt = rand(N + (D,), dtype, 3), rand(N, dtype, 4)
    adj = StandInAdjoint(core, ops, meth, setup)
    out = []
    for route in ("rollout", "chained"):
        u0 = rand(N + (D,), dtype, 1).requires_grad_(True)
        t0 = rand(N, dtype, 2).requires_grad_(True) if with_temp else None
        st = ins.create_stepper(meth, setup=setup, psolver=None, u=u0, temp=t0, t=0.25, n=3)
        if route == "rollout":
            _, ev = core.checkpoint_interval(ops, nsteps, every)
            st = core.timesteps(ops, meth, st, Δt, nsteps, ev, adj=adj)
            assert st.u.grad_fn is not None and (st.temp is None) == (not with_temp)
        else:
            for _ in range(nsteps):
                st = core.timestep(ops, meth, st, Δt, None)
        assert st.n == 3 + nsteps and st.t == pytest.approx(0.25 + nsteps * Δt)
        loss = (st.u * st.u * w).sum() + ((st.temp * st.temp * wt).sum() if with_temp else 0)
        loss.backward()
        out.append([x for x in (st.u.detach(), st.temp.detach() if with_temp else None, u0.grad, t0.grad if with_temp else None) if x is not None])
    for a, b in zip(*out):
        assert a.dtype == dtype and close(a, b, dtype)
    # forward: one call per chunk; backward: every chunk recomputes its step-start states one step at a time, then one pullback per step
    ev = min(every, nsteps)
    chunks = [min(ev, nsteps - s) for s in range(0, nsteps, ev)]
    expect = [("steps", n) for n in chunks]
    for n in reversed(chunks):
        expect += [("steps", 1)] * (n - 1) + [("pullback",)] * n
    assert adj.log == expect


@pytest.mark.parametrize("which", [0, 1])
def test_timesteps_with_one_input_requiring_grad(which):
    """Only u0 or only temp0 requires grad: its gradient is the one of the run in which both do, bit for bit; without grad nothing is saved."""
    import ins_amd as ins

    core = ins._autodiff_core
    dtype, D = torch.float64, 2
    setup, ops = make(D, dtype, True)
    ops.rk_copy_ = lambda dst, src, s, vector: dst.copy_(src)
    meth = ins.RKMethods.RK44()
    N = SHAPES[D]
    w, wt = rand(N + (D,), dtype, 3), rand(N, dtype, 4)
    adj = StandInAdjoint(core, ops, meth, setup)

    def run(req):
        xs = [rand(N + (D,), dtype, 1).requires_grad_(req[0]), rand(N, dtype, 2).requires_grad_(req[1])]
        st = core.timesteps(ops, meth, ins.create_stepper(meth, setup=setup, psolver=None, u=xs[0], temp=xs[1]), 0.05, 3, 2, adj=adj)
        if any(req):
            ((st.u * st.u * w).sum() + (st.temp * st.temp * wt).sum()).backward()
        return st, xs

    _, both = run((True, True))
    _, one = run(tuple(q == which for q in range(2)))
    assert one[1 - which].grad is None and torch.equal(one[which].grad, both[which].grad)
    st, _ = run((False, False))
    assert st.u.grad_fn is None and st.temp.grad_fn is None
