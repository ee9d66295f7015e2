"""GPU: the Float32 pullback kernels (csrc/ins_adjoint32.hip) and `ins_amd.ad32`.

Every yardstick is existing code: the fp64 pullbacks and forwards, and the existing Float32 forwards (momentum32_, project32_, timestep32_).

  1. transpose identities |<L v, w> - <v, L^T w>| / (|L v| |w|), dots in float64 from the float results, on fields with random ghost values;
  2. value by value against the fp64 twin on the same inputs promoted to double (max-norm, relative to max|result|);
  3. ad32.timestep: forward against timestep32_, gradients against the fp64 ad.timestep, a Taylor test, a torch closure;
  4. refusals.

Bounds.  The ghost-fill pullbacks add at most D ghost cotangents into a value, so |r32 - r64| <= D 2^-24 sum|terms| elementwise.  The stencil
pullbacks are held to 4 x the error of the existing Float32 FORWARD of the same stencil against its fp64 twin, measured in the same test on the
same geometry and inputs (momentum32_ against momentum_; project32_ against project_ for the projection and for the divergence and gradient
adjoints, whose chain it contains): the flux pullback gathers both product-rule branches, about twice the forward's products, and the maxima
are taken over different random fields.

The fields are random multiples of 2^-10 (float32-representable, and so are u + v and u - v) over the whole padded array.

The two families treat ghost volumes differently inside project (the Float32 spectral solver reads periodic images and refills the ghosts), so the
forward yardstick of the projection, and the value comparison for that solver, are taken on bc . project . bc — the map a time step applies, the same
in both families — whose transpose is bc^T . project^T . bc^T.  The transpose identity (1.) is on the bare project32_ / project_pullback32_.

Every test prints its figures (`RATIO ...`: measured error / forward yardstick) before it asserts.
"""
import ctypes as C

import numpy as np
import pytest

from tests import fixtures as fx

pytestmark = pytest.mark.gpu

EPS32 = 2.0**-24
MARGIN = 4.0


@pytest.fixture(scope="module")
def ins():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ins_amd

    return ins_amd


def mirror(ins, so, o):
    cls = {"PeriodicBC": ins.PeriodicBC, "SymmetricBC": ins.SymmetricBC, "PressureBC": ins.PressureBC}

    def conv(b):
        return ins.DirichletBC(b.u) if isinstance(b, o.DirichletBC) else cls[type(b).__name__]()

    bcs = tuple(tuple(conv(b) for b in side) for side in so.boundary_conditions)
    xin = []
    for a in range(so.grid.D):
        lo = 2 if isinstance(so.boundary_conditions[a][0], o.PressureBC) else 1
        xin.append(so.grid.x[a][lo:-1])
    return ins.Setup(x=xin, boundary_conditions=bcs, Re=so.Re)


def bcbox(o, kind):
    x = (np.linspace(0.0, 1.0, 8), np.linspace(0.0, 1.0, 8))
    bc = getattr(o, kind)()
    return o.make_setup(x, ((bc, bc), (bc, bc)), Re=1000.0)


def box70(o):
    """70 x 6 x 4 volumes, Dirichlet in x and y, periodic in z: the ragged second 64-wide tile, the ghost column across a wavefront boundary."""
    x = (np.linspace(0.0, 7.0, 71), np.linspace(0.0, 0.6, 7), np.linspace(0.0, 0.4, 5))
    d = (o.DirichletBC(), o.DirichletBC())
    return o.make_setup(x, (d, d, (o.PeriodicBC(), o.PeriodicBC())), Re=1000.0)


GEOMS = {
    "setup2d": fx.setup2d,
    "setup3d": fx.setup3d,
    "mixed": fx.setup_mixed,
    "box_periodic": lambda o: bcbox(o, "PeriodicBC"),
    "box_dirichlet": lambda o: bcbox(o, "DirichletBC"),
    "box_symmetric": lambda o: bcbox(o, "SymmetricBC"),
    "box_pressure": lambda o: bcbox(o, "PressureBC"),
    "periodic32_2d": lambda o: fx.setup_periodic(o, 32, D=2),
    "periodic32_3d": lambda o: fx.setup_periodic(o, 32, D=3),
    "box70": box70,
}


# ------------------------------------------------------------------------------------ helpers
def pair(ins, sp, vector, seed):
    """The same random field, multiples of 2^-10, as a float32 and as a float64 device field."""
    g = sp.grid
    shape = tuple(g.N) + ((g.dimension,) if vector else ())
    a = np.round(fx.randn_field(shape, seed) * 1024.0) / 1024.0
    return ins.f32.to_f32(sp, a), ins.from_numpy(sp, a)


def c32(ins, f):
    return ins.copyfield(f)


def dot(a, b):
    return float((a.double() * b.double()).sum().item())


def nrm(a):
    return float(a.double().norm().item())


def relmax(got, ref):
    return float((got.double() - ref).abs().max().item()) / float(ref.abs().max().item())


def rell2(got, ref):
    return float((got.double() - ref.double()).norm().item()) / float(ref.double().norm().item())


def defect(Lv, v, w, LTw):
    scale = nrm(Lv) * nrm(w)
    assert scale > 0
    return abs(dot(Lv, w) - dot(v, LTw)) / scale


def solver_pairs(ins, sp, name):
    """(label, Float32 solver, its fp64 twin)"""
    d64 = ins.psolver_direct(sp)
    out = [("wrap_direct", ins.f32.psolver_wrap32(sp, d64), d64)]
    if name.startswith("periodic32"):
        out.append(("spectral", ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)))
    return out


def step_project32(ins, sp, ps, v):
    F = ins.f32
    u = F.apply_bc_u32_(c32(ins, v), sp)
    F.project32_(u, sp, ps, F.scalarfield32(sp))
    return F.apply_bc_u32_(u, sp)


def step_project64(ins, sp, ps, v):
    u = ins.apply_bc_u_(ins.copyfield(v), 0.0, sp)
    ins.project_(u, sp, ps, ins.scalarfield(sp))
    return ins.apply_bc_u_(u, 0.0, sp)


def yard_project(ins, sp, ps32, ps64, seed=101):
    """Error of the existing Float32 projection against its fp64 twin (bc . project . bc, max-norm relative)."""
    v32, v64 = pair(ins, sp, True, seed)
    return relmax(step_project32(ins, sp, ps32, v32), step_project64(ins, sp, ps64, v64))


def yard_momentum(ins, sp, seed=102):
    u32, u64 = pair(ins, sp, True, seed)
    F = ins.f32
    return relmax(F.momentum32_(F.vectorfield32(sp), u32, sp), ins.momentum(u64, None, 0.0, sp))


def report(name, what, err, yard):
    print(f"RATIO {name} {what} err={err:.3e} yardstick={yard:.3e} ratio={err / yard:.3f}")


# ------------------------------------------------------------------------------------ 1. transpose identities
@pytest.mark.parametrize("name", list(GEOMS))
def test_transpose_identities(ins, oracle, name):
    check_transpose_identities(ins, mirror(ins, GEOMS[name](oracle), oracle), name)


def check_transpose_identities(ins, sp, name):
    """`name` labels the printed figures; a name that starts with "periodic32" adds the spectral solver pair (solver_pairs)."""
    F = ins.f32
    D = sp.grid.dimension
    v32, v64 = pair(ins, sp, True, 1)
    w32, w64 = pair(ins, sp, True, 2)
    p32, p64 = pair(ins, sp, False, 3)
    q32, q64 = pair(ins, sp, False, 4)
    pairs = solver_pairs(ins, sp, name)
    yards = {label: yard_project(ins, sp, a, b) for label, a, b in pairs}
    Ep = yards["wrap_direct"]
    results = []
    # divergence and pressure gradient: the fp64 forwards on the float-representable fields against the float adjoints
    results.append(("divergence_adjoint", defect(ins.divergence(v64, sp), v64, q64, F.divergence_adjoint32_(F.vectorfield32(sp), q32, sp)), Ep))
    results.append(("pressuregradient_adjoint", defect(ins.pressuregradient(p64, sp), p64, w64,
                                                        F.pressuregradient_adjoint32_(F.scalarfield32(sp), w32, sp)), Ep))
    # momentum is quadratic: (f(u+v) - f(u-v))/2 = J(u) v, with u + v and u - v exact in float
    u32, _ = pair(ins, sp, True, 5)
    Jv = (F.momentum32_(F.vectorfield32(sp), u32 + v32, sp).double() - F.momentum32_(F.vectorfield32(sp), u32 - v32, sp).double()) / 2
    results.append(("momentum_pullback", defect(Jv, v64, w64, F.momentum_pullback32_(F.vectorfield32(sp), w32, u32, sp)), yard_momentum(ins, sp)))
    # the projection, on each kind of solver
    for label, ps32, _ in pairs:
        Pv = F.project32_(c32(ins, v32), sp, ps32, F.scalarfield32(sp))
        PTw = F.project_pullback32_(c32(ins, w32), sp, ps32, F.scalarfield32(sp))
        results.append((f"project_pullback[{label}]", defect(Pv, v64, w64, PTw), yards[label]))
    for what, err, yard in results:
        report(name, "transpose " + what, err, yard)
    # affine ghost fills: L v = bc(v) - bc(0); the fill copies exactly, the pullback's float sums round: D 2^-24 <|v|, L^T|w|>
    Lv = F.apply_bc_u32_(c32(ins, v32), sp) - F.apply_bc_u32_(F.vectorfield32(sp), sp)
    LTw = F.apply_bc_u_pullback32_(c32(ins, w32), sp)
    bound_u = D * EPS32 * dot(v64.abs(), ins.apply_bc_u_pullback_(w64.abs(), 0.0, sp))
    du = abs(dot(Lv, w64) - dot(v64, LTw))
    Lp = F.apply_bc_p32_(c32(ins, p32), sp) - F.apply_bc_p32_(F.scalarfield32(sp), sp)
    LTq = F.apply_bc_p_pullback32_(c32(ins, q32), sp)
    bound_p = D * EPS32 * dot(p64.abs(), ins.apply_bc_p_pullback_(q64.abs(), 0.0, sp))
    dp = abs(dot(Lp, q64) - dot(p64, LTq))
    print(f"RATIO {name} transpose apply_bc_u defect={du:.3e} bound={bound_u:.3e}; apply_bc_p defect={dp:.3e} bound={bound_p:.3e}")
    assert nrm(Lv) > 0 and du <= bound_u
    assert dp <= bound_p
    for what, err, yard in results:
        assert err <= MARGIN * yard, (what, err, yard)


# ------------------------------------------------------------------------------------ 2. values against the fp64 twins
@pytest.mark.parametrize("name", list(GEOMS))
def test_values_against_fp64(ins, oracle, name):
    check_values_against_fp64(ins, mirror(ins, GEOMS[name](oracle), oracle), name)


def check_values_against_fp64(ins, sp, name):
    F = ins.f32
    D = sp.grid.dimension
    u32, u64 = pair(ins, sp, True, 11)
    w32, w64 = pair(ins, sp, True, 12)
    q32, q64 = pair(ins, sp, False, 13)
    b32, b64 = pair(ins, sp, True, 14)
    pairs = solver_pairs(ins, sp, name)
    yards = {label: yard_project(ins, sp, a, b) for label, a, b in pairs}
    Ep, Em = yards["wrap_direct"], yard_momentum(ins, sp)
    results = []
    r64 = ins.momentum_pullback_(ins.vectorfield(sp), w64, u64, sp)
    results.append(("momentum_pullback", relmax(F.momentum_pullback32_(F.vectorfield32(sp), w32, u32, sp), r64), Em))
    results.append(("momentum_pullback[accumulate]", relmax(F.momentum_pullback32_(c32(ins, b32), w32, u32, sp, accumulate=True), b64 + r64), Em))
    results.append(("divergence_adjoint", relmax(F.divergence_adjoint32_(F.vectorfield32(sp), q32, sp),
                                                 ins.divergence_adjoint_(ins.vectorfield(sp), q64, sp)), Ep))
    results.append(("pressuregradient_adjoint", relmax(F.pressuregradient_adjoint32_(F.scalarfield32(sp), w32, sp),
                                                       ins.pressuregradient_adjoint_(ins.scalarfield(sp), w64, sp)), Ep))
    for label, ps32, ps64 in pairs:
        if label == "wrap_direct":  # the same chain as ins_project_pullback_f64 on the padded array
            got = F.project_pullback32_(c32(ins, w32), sp, ps32, F.scalarfield32(sp))
            ref = ins.project_pullback_(ins.copyfield(w64), sp, ps64, ins.scalarfield(sp))
            results.append((f"project_pullback[{label}]", relmax(got, ref), yards[label]))
        got = F.apply_bc_u_pullback32_(c32(ins, w32), sp)
        F.project_pullback32_(got, sp, ps32, F.scalarfield32(sp))
        F.apply_bc_u_pullback32_(got, sp)
        ref = ins.apply_bc_u_pullback_(ins.copyfield(w64), 0.0, sp)
        ins.project_pullback_(ref, sp, ps64, ins.scalarfield(sp))
        ins.apply_bc_u_pullback_(ref, 0.0, sp)
        results.append((f"bcT.project_pullback.bcT[{label}]", relmax(got, ref), yards[label]))
    for what, err, yard in results:
        report(name, "value " + what, err, yard)
    # ghost fills, elementwise: |r32 - r64| <= D 2^-24 sum|terms|, the sum of the terms' magnitudes being the fp64 pullback of |w|
    gu = (F.apply_bc_u_pullback32_(c32(ins, w32), sp).double() - ins.apply_bc_u_pullback_(ins.copyfield(w64), 0.0, sp)).abs()
    assert bool((gu <= D * EPS32 * ins.apply_bc_u_pullback_(w64.abs(), 0.0, sp)).all())
    gp = (F.apply_bc_p_pullback32_(c32(ins, q32), sp).double() - ins.apply_bc_p_pullback_(ins.copyfield(q64), 0.0, sp)).abs()
    assert bool((gp <= D * EPS32 * ins.apply_bc_p_pullback_(q64.abs(), 0.0, sp)).all())
    for what, err, yard in results:
        assert err <= MARGIN * yard, (what, err, yard)


# ------------------------------------------------------------------------------------ 3. ad32.timestep
DT, NSTEP = 1e-3, 3
STEP_CASES = [("periodic32_2d", "spectral"), ("mixed", "wrap_direct")]


def _solvers_for_step(ins, sp, kind):
    if kind == "spectral":
        return ins.f32.psolver_spectral32(sp), ins.psolver_spectral(sp)
    d64 = ins.psolver_direct(sp)
    return ins.f32.psolver_wrap32(sp, d64), ins.psolver_direct(sp)


def _u0(ins, sp, ps64, seed):
    """A ghost-filled, divergence-free start field, float32-representable, in both precisions."""
    _, r = pair(ins, sp, True, seed)
    u = ins.apply_bc_u_(ins.project_(ins.apply_bc_u_(r, 0.0, sp), sp, ps64, ins.scalarfield(sp)), 0.0, sp)
    u32 = ins.f32.to_f32(sp, u)
    u64 = ins.copyfield(u)
    u64.copy_(u32)
    return u32, u64


def _steps(ins, ad, sp, ps, u, θ=None):
    method = ins.RKMethods.RK44()
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u)
    for _ in range(NSTEP):
        st = ad.timestep(method, st, DT, θ=θ)
    return st.u


def _ke(u):
    return 0.5 * (u.double() * u.double()).sum()


@pytest.mark.parametrize("name,kind", STEP_CASES)
def test_timestep_forward_and_gradient(ins, oracle, name, kind):
    import torch

    sp = mirror(ins, GEOMS[name](oracle), oracle)
    ps32, ps64 = _solvers_for_step(ins, sp, kind)
    u32, u64 = _u0(ins, sp, ps64, 40)
    method = ins.RKMethods.RK44()
    # forward: fp64 native, Float32 native, ad32
    ref64 = ins.copyfield(u64)
    st = ins.create_stepper(method, setup=sp, psolver=ps64, u=ref64)
    for _ in range(NSTEP):
        st = ins.timestep(method, st, DT)
    ref64 = st.u
    nat32 = c32(ins, u32)
    cache = ins.f32.ERKCache32(method, sp, ps32)
    for _ in range(NSTEP):
        ins.f32.timestep32_(cache, nat32, DT)
    yard_native = rell2(nat32, ref64)
    uu32 = u32.clone().requires_grad_(True)
    out32 = _steps(ins, ins.ad32, sp, ps32, uu32)
    fwd = rell2(out32.detach(), nat32)
    yard = rell2(out32.detach(), ref64)
    print(f"RATIO {name} timestep forward ad32-vs-timestep32_={fwd:.3e} timestep32_-vs-fp64={yard_native:.3e} ad32-vs-fp64={yard:.3e} "
          f"bitwise={bool((out32.detach() == nat32).all())}")
    # gradient of 1/2 |u_N|^2 with respect to u0 against the fp64 ad.timestep
    (g32,) = torch.autograd.grad(_ke(out32), uu32)
    uu64 = u64.clone().requires_grad_(True)
    (g64,) = torch.autograd.grad(_ke(_steps(ins, ins.ad, sp, ps64, uu64)), uu64)
    gerr = rell2(g32, g64)
    report(name, "timestep gradient_u0", gerr, yard)
    assert g32.dtype == torch.float32 and float(g64.norm()) > 0
    # two Float32 evaluations of the same step that differ only in the rounding of the stage combinations: each is one Float32 step away from fp64
    assert fwd <= MARGIN * yard_native, (fwd, yard_native)
    assert gerr <= MARGIN * yard, (gerr, yard)


def test_timestep_taylor(ins, oracle):
    """First-order Taylor remainder of J(u0 + h v) in Float32, at step sizes whose second-order term is far above the rounding of J."""
    import torch

    name, kind = STEP_CASES[0]
    sp = mirror(ins, GEOMS[name](oracle), oracle)
    ps32, ps64 = _solvers_for_step(ins, sp, kind)
    u32, u64 = _u0(ins, sp, ps64, 41)
    v32, _ = _u0(ins, sp, ps64, 42)
    v32 = v32 * (float(u32.norm()) / float(v32.norm()))
    uu = u32.clone().requires_grad_(True)
    J0t = _ke(_steps(ins, ins.ad32, sp, ps32, uu))
    (g,) = torch.autograd.grad(J0t, uu)
    J0, dJ = float(J0t), dot(g, v32)
    with torch.no_grad():
        noise = abs(J0 - float(_ke(_steps(ins, ins.ad, sp, ps64, u64))))  # the forward rounding of J
        hs = [0.2, 0.1, 0.05]  # second-order term ~ h^2 J0 (|v| = |u0|): 4e-2 .. 2.5e-3 of J0, rounding ~ 1e-7 of J0
        r = [abs(float(_ke(_steps(ins, ins.ad32, sp, ps32, u32 + h * v32))) - J0 - h * dJ) for h in hs]
    ratios = [r[k] / r[k + 1] for k in range(2)]
    print(f"RATIO {name} taylor J0={J0:.6e} dJ={dJ:.6e} noise={noise:.3e} remainders={r} ratios={ratios}")
    assert min(r) > 100 * noise, (r, noise)
    assert all(3.0 <= x <= 5.0 for x in ratios), (r, ratios)


def test_timestep_closure_gradient(ins, oracle):
    """A torch closure m(u, θ) in float32 (neuralclosure.cnn cast to float): ∂/∂θ against the fp64 ad.timestep of the same network in double."""
    import copy

    import torch

    name, kind = STEP_CASES[0]
    sp32 = mirror(ins, GEOMS[name](oracle), oracle)
    sp64 = mirror(ins, GEOMS[name](oracle), oracle)
    net64 = ins.cnn(setup=sp64, radii=[1, 1], channels=[4, 2], activations=[torch.tanh, None], use_bias=[True, False], rng=7)
    net32 = copy.deepcopy(net64).float()
    with torch.no_grad():
        for a, b in zip(net64.parameters(), net32.parameters()):
            a.copy_(b)  # float32-representable weights in both
    sp32.closure_model = ins.wrappedclosure(net32, sp32)
    sp64.closure_model = ins.wrappedclosure(net64, sp64)
    ps32, ps64 = _solvers_for_step(ins, sp32, kind)[0], ins.psolver_spectral(sp64)
    u32, u64 = _u0(ins, sp64, ps64, 43)
    out32 = _steps(ins, ins.ad32, sp32, ps32, u32)
    out64 = _steps(ins, ins.ad, sp64, ps64, u64)
    yard = rell2(out32.detach(), out64.detach())
    g32 = torch.autograd.grad(_ke(out32), list(net32.parameters()))
    g64 = torch.autograd.grad(_ke(out64), list(net64.parameters()))
    f32v = torch.cat([x.reshape(-1).double() for x in g32])
    f64v = torch.cat([x.reshape(-1) for x in g64])
    gerr = float((f32v - f64v).norm()) / float(f64v.norm())
    report(name, "timestep gradient_theta", gerr, yard)
    assert all(x.dtype == torch.float32 for x in g32)
    assert bool(torch.isfinite(f32v).all()) and float(f32v.norm()) > 0
    assert gerr <= MARGIN * yard, (gerr, yard)


# ------------------------------------------------------------------------------------ 4. refusals
def test_ad32_refusals(ins):
    F = ins.f32
    x = (np.linspace(0.0, 1.0, 17), np.linspace(0.0, 1.0, 17))
    method = ins.RKMethods.RK44()
    per = (ins.PeriodicBC(), ins.PeriodicBC())

    def step(sp, ps, temp=None):
        st = ins.create_stepper(method, setup=sp, psolver=ps, u=F.vectorfield32(sp), temp=temp)
        return ins.ad32.timestep(method, st, 1e-3)

    sp = ins.Setup(x=x, Re=100.0)
    ps = F.psolver_spectral32(sp)
    step(sp, ps)  # the plain setup runs
    with pytest.raises(NotImplementedError):  # a temperature field
        step(sp, ps, temp=F.scalarfield32(sp))
    with pytest.raises(NotImplementedError):
        ins.ad32.momentum(F.vectorfield32(sp), F.scalarfield32(sp), 0.0, sp)
    with pytest.raises(NotImplementedError):  # wrapped spectral solver on an all-periodic box
        step(sp, F.psolver_wrap32(sp, ins.psolver_spectral(sp)))
    with pytest.raises(NotImplementedError):
        ins.ad32.project(F.vectorfield32(sp), sp, F.psolver_wrap32(sp, ins.psolver_spectral(sp)))
    sp.closure_model = ins.smagorinsky_closure(sp)  # the library's fused Smagorinsky closure
    with pytest.raises(NotImplementedError):
        step(sp, ps)
    sp.closure_model = None
    spf = ins.Setup(x=x, Re=100.0, bodyforce=lambda a, xx, yy, t: np.sin(xx + t) * (a == 0) + 0 * yy, issteadybodyforce=False)
    with pytest.raises(NotImplementedError):  # an unsteady body force
        step(spf, F.psolver_spectral32(spf))
    lid = ins.DirichletBC(lambda a, xx, yy, t: (a == 0) * np.cos(t) + 0 * xx * yy)
    spc = ins.Setup(x=x, Re=100.0, boundary_conditions=((ins.DirichletBC(), ins.DirichletBC()), (ins.DirichletBC(), lid)))
    with pytest.raises(NotImplementedError):  # callable boundary data
        ins.ad32.apply_bc_u(F.vectorfield32(spc), 0.0, spc)
    x3 = tuple(np.linspace(0.0, 1.0, 9) for _ in range(3))
    slab = ins.Setup(x=x3, Re=100.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    with pytest.raises(NotImplementedError):  # slab setups
        ins.ad32.apply_bc_u(F.vectorfield32(slab), 0.0, slab)
    with pytest.raises(NotImplementedError):
        ins.ad32.momentum(F.vectorfield32(slab), None, 0.0, slab)


def test_c_entry_points_refuse(ins):
    """INS_ERR_UNSUPPORTED (-4) on a slab grid; INS_ERR_INVALID (-1) for the in-place momentum pullback.  (No Float32 solver handle can be made for
    a slab grid, so ins_project_pullback_f32 is reached there only with a solver of another grid: INS_ERR_INVALID.)"""
    F = ins.f32
    lib = ins._lib.load()
    per = (ins.PeriodicBC(), ins.PeriodicBC())
    x3 = tuple(np.linspace(0.0, 1.0, 9) for _ in range(3))
    slab = ins.Setup(x=x3, Re=100.0, boundary_conditions=(per, per, (ins.HaloBC(), ins.HaloBC())))
    u, w, ub, p = F.vectorfield32(slab), F.vectorfield32(slab), F.vectorfield32(slab), F.scalarfield32(slab)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    h, s = slab.handle, slab.stream
    assert lib.ins_divergence_adjoint_f32(h, vp(p), vp(ub), s) == -4
    assert b"slab" in lib.ins_last_error()
    assert lib.ins_pressuregradient_adjoint_f32(h, vp(w), vp(p), s) == -4
    assert lib.ins_momentum_pullback_f32(h, 0.01, vp(u), vp(w), vp(ub), 0, s) == -4
    assert lib.ins_apply_bc_u_pullback_f32(h, vp(w), s) == -4
    assert lib.ins_apply_bc_p_pullback_f32(h, vp(p), s) == -4
    box = ins.Setup(x=x3, Re=100.0)
    ps = F.psolver_spectral32(box)
    assert lib.ins_project_pullback_f32(h, ps.handle, vp(w), vp(p), s) == -1
    u, w = F.vectorfield32(box), F.vectorfield32(box)
    hb, sb = box.handle, box.stream
    assert lib.ins_momentum_pullback_f32(hb, 0.01, vp(u), vp(w), vp(u), 0, sb) == -1
    assert lib.ins_momentum_pullback_f32(hb, 0.01, vp(u), vp(w), vp(w), 1, sb) == -1
    with pytest.raises(ins.INSHipError):
        F.momentum_pullback32_(u, w, u, box)
    wrapped = F.psolver_wrap32(box, ins.psolver_spectral(box))
    assert lib.ins_project_pullback_f32(hb, wrapped.handle, vp(w), vp(F.scalarfield32(box)), sb) == -4
