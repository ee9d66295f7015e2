"""GPU: the pullback kernels (csrc/ins_adjoint.hip) and `ins_amd.ad`.

  1. transpose identities |<L v, w> - <v, L^T w>| <= tol |L v| |w| over the whole padded arrays, for every linear pullback;
  2. convection / momentum / right_hand_side are quadratic, so (f(u+v) - f(u-v))/2 = J(u) v exactly and the same identity holds for J(u)^T;
  3. value by value against the dense transpose of the CPU oracle's forward operators (unit probes);
  4. torch.autograd: gradcheck, ad.timestep against the native step, Taylor tests through 20 RK44 steps (in u0 and in closure parameters).
"""
import numpy as np
import pytest

from tests import fixtures as fx

pytestmark = pytest.mark.gpu

TOL = 1e-12


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
    """test/chainrules.jl:12-35: 7 x 7 on [0, 1]^2, one BC type on every side."""
    x = (np.linspace(0.0, 1.0, 8), np.linspace(0.0, 1.0, 8))
    bc = getattr(o, kind)()
    return o.make_setup(x, ((bc, bc), (bc, bc)), Re=1000.0)


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
}
ORACLE_GEOMS = ["mixed", "box_periodic", "box_dirichlet", "box_symmetric", "box_pressure"]


def rand(ins, sp, vector, seed):
    g = sp.grid
    shape = tuple(g.N) + ((g.dimension,) if vector else ())
    return ins.from_numpy(sp, fx.randn_field(shape, seed))


def dot(a, b):
    return float((a * b).sum().item())


def nrm(a):
    return float(a.norm().item())


def check_transpose(Lv, v, w, LTw, tol=TOL):
    lhs, rhs = dot(Lv, w), dot(v, LTw)
    scale = nrm(Lv) * nrm(w)
    assert scale > 0
    assert abs(lhs - rhs) <= tol * scale, (lhs, rhs, abs(lhs - rhs) / scale)


def solvers(ins, sp, name):
    if name.startswith("periodic"):  # the 7 x 7 box has an odd number of volumes: no spectral solver
        return [ins.psolver_spectral(sp), ins.psolver_direct(sp)]
    return [ins.psolver_direct(sp)]


# ------------------------------------------------------------------------------------ 1. transpose identities
@pytest.mark.parametrize("name", list(GEOMS))
def test_linear_transposes(ins, oracle, name):
    sp = mirror(ins, GEOMS[name](oracle), oracle)
    check_linear_transposes(ins, sp, solvers(ins, sp, name))


def check_linear_transposes(ins, sp, pss):
    """Every linear pullback of setup `sp`; the Poisson solve and the projection on each solver of `pss`."""
    z = ins.vectorfield(sp)
    v, w = rand(ins, sp, True, 1), rand(ins, sp, True, 2)
    p, q = rand(ins, sp, False, 3), rand(ins, sp, False, 4)
    # divergence: u -> p
    check_transpose(ins.divergence(v, sp), v, q, ins.divergence_adjoint_(ins.vectorfield(sp), q, sp))
    # pressuregradient: p -> u
    check_transpose(ins.pressuregradient(p, sp), p, w, ins.pressuregradient_adjoint_(ins.scalarfield(sp), w, sp))
    # diffusion (both viscosity switches)
    for uv in (True, False):
        check_transpose(ins.diffusion(v, sp, uv), v, w, ins.diffusion_adjoint_(ins.vectorfield(sp), w, sp, uv))
    # affine ghost fills: L v = bc(v) - bc(0)
    Lv = ins.apply_bc_u(v, 0.0, sp) - ins.apply_bc_u(z, 0.0, sp)
    check_transpose(Lv, v, w, ins.apply_bc_u_pullback_(ins.copyfield(w), 0.0, sp))
    Lp = ins.apply_bc_p(p, 0.0, sp) - ins.apply_bc_p(ins.scalarfield(sp), 0.0, sp)
    check_transpose(Lp, p, q, ins.apply_bc_p_pullback_(ins.copyfield(q), 0.0, sp))
    # applypressure (u, p) -> u - G p through autograd: <w, u - Gp> = <ubar, u> + <pbar, p>
    vv, pp = v.clone().requires_grad_(True), p.clone().requires_grad_(True)
    out = ins.ad.applypressure(vv, pp, sp)
    ub, pb = __import__("torch").autograd.grad(out, (vv, pp), w)
    lhs = dot(out.detach(), w)
    assert abs(lhs - dot(ub, v) - dot(pb, p)) <= TOL * nrm(out.detach()) * nrm(w)
    # the Poisson solve and the projection
    for ps in pss:
        check_transpose(ps(ins.copyfield(p)), p, q, ps(ins.copyfield(q)))
        Pv = ins.project_(ins.copyfield(v), sp, ps, ins.scalarfield(sp))
        check_transpose(Pv, v, w, ins.project_pullback_(ins.copyfield(w), sp, ps, ins.scalarfield(sp)))


def test_project_transpose_cg(ins, oracle):
    sp = mirror(ins, fx.setup2d(oracle), oracle)
    ps = ins.psolver_cg(sp, reltol=1e-13)
    # all-Dirichlet: the Poisson system is singular, so CG needs a compatible right-hand side — a v whose ghost normal velocities are the
    # (zero) boundary data.  The pullback's own right-hand side bc_p^T G^T w always is one (<1, G^T w> = <G 1, w> = 0).
    v, w = ins.apply_bc_u(rand(ins, sp, True, 5), 0.0, sp), rand(ins, sp, True, 6)
    Pv = ins.project_(ins.copyfield(v), sp, ps, ins.scalarfield(sp))
    check_transpose(Pv, v, w, ins.project_pullback_(ins.copyfield(w), sp, ps, ins.scalarfield(sp)), tol=1e-6)


# ------------------------------------------------------------------------------------ 2. quadratic operators
@pytest.mark.parametrize("name", list(GEOMS))
def test_convection_and_momentum_pullbacks(ins, oracle, name):
    check_convection_and_momentum_pullbacks(ins, mirror(ins, GEOMS[name](oracle), oracle))


def check_convection_and_momentum_pullbacks(ins, sp):
    u, v, w = rand(ins, sp, True, 7), rand(ins, sp, True, 8), rand(ins, sp, True, 9)
    Jv = (ins.convection(u + v, sp) - ins.convection(u - v, sp)) / 2
    ub = ins.convection_adjoint_(ins.vectorfield(sp), w, u, sp)
    check_transpose(Jv, v, w, ub)
    Mv = (ins.momentum(u + v, None, 0.0, sp) - ins.momentum(u - v, None, 0.0, sp)) / 2
    mb = ins.momentum_pullback_(ins.vectorfield(sp), w, u, sp)
    check_transpose(Mv, v, w, mb)
    # the fused pass equals convection + diffusion pullbacks; accumulate adds
    ref = ins.diffusion_adjoint_(ins.convection_adjoint_(ins.vectorfield(sp), w, u, sp), w, sp)
    assert float((mb - ref).abs().max()) <= TOL * float(ref.abs().max())
    acc = ins.momentum_pullback_(ins.copyfield(ref), w, u, sp, accumulate=True)
    assert float((acc - 2 * ref).abs().max()) <= TOL * float(ref.abs().max())


@pytest.mark.parametrize("name", ["setup2d", "mixed", "box_periodic", "box_symmetric", "box_pressure", "periodic32_2d", "periodic32_3d"])
def test_right_hand_side_pullback(ins, oracle, name):
    import torch

    sp = mirror(ins, GEOMS[name](oracle), oracle)
    u, v, w = rand(ins, sp, True, 10), rand(ins, sp, True, 11), rand(ins, sp, True, 12)
    for ps in solvers(ins, sp, name):
        rhs = ins.ad.create_right_hand_side(sp, ps)
        with torch.no_grad():
            Jv = (rhs(u + v, None, 0.0) - rhs(u - v, None, 0.0)) / 2
        uu = u.clone().requires_grad_(True)
        out = rhs(uu, None, 0.0)
        (ub,) = torch.autograd.grad(out, uu, w)
        check_transpose(Jv, v, w, ub, tol=1e-11)
        # forward equals the library's in-place right-hand side
        ref = ins.vectorfield(sp)
        ins.right_hand_side_(ref, u, (sp, ps), 0.0)
        assert float((out.detach() - ref).abs().max()) <= TOL * float(ref.abs().max())


# ------------------------------------------------------------------------------------ 3. against the oracle, value by value
def dense_transpose_apply(L, shape, w):
    """(dL)^T w of a linear map L on numpy fields of `shape`, by unit probes."""
    n = int(np.prod(shape))
    wf = w.reshape(-1, order="F")
    out = np.empty(n)
    e = np.zeros(n)
    for k in range(n):
        e[k] = 1.0
        out[k] = np.dot(wf, L(e.reshape(shape, order="F")).reshape(-1, order="F"))
        e[k] = 0.0
    return out.reshape(shape, order="F")


def relmax(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("name", ORACLE_GEOMS)
def test_pullbacks_match_oracle_transposes(ins, oracle, name):
    o = oracle
    so = GEOMS[name](o)
    sp = mirror(ins, so, o)
    for what, L, shape, cot, got in oracle_transpose_cases(ins, o, so, sp):
        ref = dense_transpose_apply(L, shape, cot)
        err = relmax(ins.to_numpy(got), ref)
        assert err <= TOL, (what, err)


def oracle_transpose_cases(ins, o, so, sp):
    """(name, the oracle's linear map L, shape of its argument, cotangent, the library's L^T cotangent) of every pullback that has an oracle forward"""
    N, D = tuple(so.grid.N), so.grid.D
    vs, ss = N + (D,), N
    u = fx.randn_field(vs, 20)
    w, q = fx.randn_field(vs, 21), fx.randn_field(ss, 22)
    ug, wg, qg = ins.from_numpy(sp, u), ins.from_numpy(sp, w), ins.from_numpy(sp, q)
    z, zs = np.zeros(vs, order="F"), np.zeros(ss, order="F")
    return [
        ("divergence", lambda x: o.divergence(x, so), vs, q, ins.divergence_adjoint_(ins.vectorfield(sp), qg, sp)),
        ("pressuregradient", lambda x: o.pressuregradient(x, so), ss, w, ins.pressuregradient_adjoint_(ins.scalarfield(sp), wg, sp)),
        ("diffusion", lambda x: o.diffusion(x, so), vs, w, ins.diffusion_adjoint_(ins.vectorfield(sp), wg, sp)),
        ("convection", lambda x: (o.convection(u + x, so) - o.convection(u - x, so)) / 2, vs, w,
         ins.convection_adjoint_(ins.vectorfield(sp), wg, ug, sp)),
        ("apply_bc_u", lambda x: o.apply_bc_u(x, 0.0, so) - o.apply_bc_u(z, 0.0, so), vs, w,
         ins.apply_bc_u_pullback_(ins.copyfield(wg), 0.0, sp)),
        ("apply_bc_p", lambda x: o.apply_bc_p(x, 0.0, so) - o.apply_bc_p(zs, 0.0, so), ss, q,
         ins.apply_bc_p_pullback_(ins.copyfield(qg), 0.0, sp)),
    ]


# ------------------------------------------------------------------------------------ 4. torch.autograd
@pytest.mark.parametrize("kind", ["PeriodicBC", "DirichletBC"])
def test_gradcheck_right_hand_side(ins, oracle, kind):
    import torch

    x = (np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9))
    bc = getattr(oracle, kind)()
    sp = mirror(ins, oracle.make_setup(x, ((bc, bc), (bc, bc)), Re=100.0), oracle)
    ps = ins.default_psolver(sp)
    u = rand(ins, sp, True, 30).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda uu: ins.ad.right_hand_side(uu, (sp, ps), 0.0), (u,), eps=1e-6, atol=1e-6, rtol=1e-6)


def _u0(ins, sp, ps, seed):
    u = ins.apply_bc_u(rand(ins, sp, True, seed), 0.0, sp)
    return ins.apply_bc_u(ins.project_(u, sp, ps, ins.scalarfield(sp)), 0.0, sp)


@pytest.mark.parametrize("name", ["periodic32_3d", "mixed"])
def test_ad_timestep_forward_matches_native(ins, oracle, name):
    sp = mirror(ins, GEOMS[name](oracle), oracle)
    ps = ins.default_psolver(sp)
    method = ins.RKMethods.RK44()
    u0 = _u0(ins, sp, ps, 40)
    dt = 1e-3
    ref = ins.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), dt).u
    got = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), dt).u
    assert float((got - ref).abs().max()) <= TOL * float(ref.abs().max())


def _taylor(J, dJ, eps0):
    """Remainders |J(ε) - J(0) - ε dJ| at ε0 / 2^k, k = 0..3: each halving divides them by 4 ± 0.5."""
    J0 = J(0.0)
    r = [abs(J(eps0 / 2**k) - J0 - eps0 / 2**k * dJ) for k in range(4)]
    ratios = [r[k] / r[k + 1] for k in range(3)]
    assert all(abs(x - 4.0) <= 0.5 for x in ratios), (r, ratios)
    return J0


def _manual_setup(ins, closure_model=None):
    n = 64
    x = (np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1))
    return ins.Setup(x=x, Re=500.0, closure_model=closure_model)


def _final_ke(ins, sp, ps, u0, nstep, θ=None):
    method = ins.RKMethods.RK44()
    st = ins.create_stepper(method, setup=sp, psolver=ps, u=u0)
    for _ in range(nstep):
        st = ins.ad.timestep(method, st, 1e-3, θ=θ)
    u = st.u[1:-1, 1:-1, :]
    h = 1.0 / 64
    return 0.5 * (u * u).sum() * h * h


def test_manual_example_gradient_wrt_u0(ins):
    """docs/src/manual/differentiability.md:25-63 scaled down: gradient of the final kinetic energy after 20 RK44 steps with respect to u0."""
    import torch

    sp = _manual_setup(ins)
    ps = ins.psolver_spectral(sp)
    u0 = ins.random_field(sp, 0.0, psolver=ps, seed=3)
    v = _u0(ins, sp, ps, 50)
    v = v * (float(u0.norm()) / float(v.norm()))
    uu = u0.clone().requires_grad_(True)
    ke = _final_ke(ins, sp, ps, uu, 20)
    (g,) = torch.autograd.grad(ke, uu)
    dJ = dot(g, v)

    def J(e):
        with torch.no_grad():
            return float(_final_ke(ins, sp, ps, u0 + e * v, 20))

    _taylor(J, dJ, 1e-2)
    e = 1e-4
    fd = (J(e) - J(-e)) / (2 * e)
    assert abs(fd - dJ) <= 1e-6 * abs(dJ), (fd, dJ)


def test_closure_model_gradient_wrt_theta(ins):
    """a-posteriori training: a torch closure m(u, θ) inside ad.timestep gets ∂/∂θ from torch."""
    import torch

    def m(u, θ):
        return θ[0] * u + θ[1] * u * u

    sp = _manual_setup(ins, closure_model=m)
    ps = ins.psolver_spectral(sp)
    u0 = ins.random_field(sp, 0.0, psolver=ps, seed=4)
    θ0 = torch.tensor([-0.5, 0.2], dtype=torch.float64, device=sp.device)
    dθ = torch.tensor([0.7, -0.3], dtype=torch.float64, device=sp.device)
    th = θ0.clone().requires_grad_(True)
    ke = _final_ke(ins, sp, ps, u0, 20, th)
    (g,) = torch.autograd.grad(ke, th)
    dJ = float((g * dθ).sum())

    def J(e):
        with torch.no_grad():
            return float(_final_ke(ins, sp, ps, u0, 20, θ0 + e * dθ))

    _taylor(J, dJ, 0.2)
    e = 1e-4
    fd = (J(e) - J(-e)) / (2 * e)
    assert abs(fd - dJ) <= 1e-6 * abs(dJ), (fd, dJ)


def test_unsupported_paths_raise(ins):
    sp = _manual_setup(ins)
    sp.closure_model = ins.smagorinsky_closure(sp)
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    u0 = ins.random_field(sp, 0.0, psolver=ps, seed=5).requires_grad_(True)
    with pytest.raises(NotImplementedError):
        ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=u0), 1e-3, θ=0.1)
    with pytest.raises(NotImplementedError):
        ins.ad.momentum(u0, ins.scalarfield(sp), 0.0, sp)


# ------------------------------------------------------------------------------------ 5. tiled against generic
def _periodic_box(ins, n):
    x = tuple(np.linspace(0.0, 1.0, n + 1) for _ in range(3))
    sp = ins.Setup(x=x, Re=1000.0)
    assert ins._lib.load().ins_grid_is_uniform_exact(sp.handle), "the tiled pullback serves this box"
    return sp


def _randn_field(ins, sp, seed):
    import torch

    f = ins.vectorfield(sp)
    g = torch.Generator(device=sp.device).manual_seed(seed)
    f.copy_(torch.randn(f.shape, generator=g, dtype=torch.float64, device=sp.device))
    return f


@pytest.mark.parametrize("n", [256, 96])
def test_tiled_momentum_pullback_matches_generic(ins, n):
    sp = _periodic_box(ins, n)
    u, w = _randn_field(ins, sp, 60), _randn_field(ins, sp, 61)
    base = _randn_field(ins, sp, 62)
    res = {}
    for off in (0, 1):
        with ins._lib.options(INS_DISABLE_ADJ_TILED=off):
            res[off] = ins.momentum_pullback_(ins.vectorfield(sp), w, u, sp)
            res[off, "acc"] = ins.momentum_pullback_(ins.copyfield(base), w, u, sp, accumulate=True)
    scale = float(res[1].abs().max())
    assert float((res[0] - res[1]).abs().max()) <= TOL * scale
    assert float((res[0, "acc"] - res[1, "acc"]).abs().max()) <= TOL * float(res[1, "acc"].abs().max())
    del res, u, w, base


def test_rk44_vjp_tiled_vs_generic(ins):
    import torch

    sp = _periodic_box(ins, 64)
    ps = ins.psolver_spectral(sp)
    method = ins.RKMethods.RK44()
    u0 = ins.random_field(sp, 0.0, psolver=ps, seed=7)
    w = _randn_field(ins, sp, 63)
    grads = []
    for off in (0, 1):
        with ins._lib.options(INS_DISABLE_ADJ_TILED=off):
            uu = u0.clone().requires_grad_(True)
            u1 = ins.ad.timestep(method, ins.create_stepper(method, setup=sp, psolver=ps, u=uu), 1e-3).u
            (g,) = torch.autograd.grad(u1, uu, w)
            grads.append(g)
    assert float((grads[0] - grads[1]).abs().max()) <= TOL * float(grads[1].abs().max())


def test_saved_velocity_is_version_checked(ins):
    """ad.convection / ad.momentum keep the field they read through save_for_backward: changing it in place before backward raises."""
    import torch

    sp = _periodic_box(ins, 32)
    for f in (lambda u: ins.ad.convection(u, sp), lambda u: ins.ad.momentum(u, None, 0.0, sp)):
        u = _randn_field(ins, sp, 64).requires_grad_(True)
        out = f(u)
        with torch.no_grad():
            u.add_(1.0)
        with pytest.raises(RuntimeError):
            out.backward(torch.ones_like(out))
