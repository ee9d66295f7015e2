// Pullback of one explicit Runge-Kutta step (step_explicit_runge_kutta.jl:4-59 without closure, temperature or time-dependent boundary data) with
// respect to the field it starts from: the reverse stage loop behind `ad.timesteps` (autodiff.py), one C call per step.
//
// Forward, stage i = 0..s-1, with u_0 = ustart (A the shifted tableau, f the steady body force or 0):
//     v_i = bc(u_i)          k_i = F(v_i) + f          w_i = ustart + Δt Σ_{j<=i} A[i,j] k_j          u_{i+1} = P(bc(w_i))
// and u_out = bc(u_s).  Reverse, with g the cotangent of v_{i+1} (of u_out at the start):
//     ȳ_i = bcᵀ Pᵀ bcᵀ g  (cotangent of w_i)          k̄_i = Δt Σ_{i'>=i} A[i',i] ȳ_{i'}          g = J(v_i)ᵀ k̄_i
// and ∂L/∂ustart = Σ_i ȳ_i + bcᵀ g.  The force is additive and drops out; it enters the recomputation of the v_i only.
//
// k̄_i is written by k_weighted_sum and read back by the plain momentum pullback.  With INS_ADJ_STAGE_FUSED=1, where it has at most
// INS_ADJ_COMB_MAX terms, it is never written: the momentum pullback kernels read the ȳ_{i'} and form the combination where they load the
// cotangent (PhiComb, ins_adjoint_kernels.h).  That saves 48 B per cell and stage and measured slower on an MI355X, hence opt-in.
//
// That loop is kept as it was; with a closure set (ins_rk_adjoint_set_closure) ins_rk_step_pullback_f64 runs the generic loop instead.  The Float32
// step and the steps with a temperature (ins_rk_step_pullback_f32, ins_rk_step_pullback_ext_f64 / _f32) run the one generic loop of
// ins_rk_adjoint_loop.h, which never fuses the combination (INS_ADJ_STAGE_FUSED is ignored there).
#include "ins_adjoint_kernels.h"
#include "ins_f32_internal.h"
#include "ins_rk_adjoint_loop.h"
#include "ins_rk_terms.h"

struct ins_rk_adjoint : RkAdjointT<double, ins_poisson> {};
struct ins_rk_adjoint32 : RkAdjointT<float, ins_poisson32> {};

namespace {

struct WeightedSum {
  int n;
  double w[INS_MAX_STAGES];
  const double* p[INS_MAX_STAGES];
};

// out = Σ_q w[q]·p[q] over a whole vector field (the two-launch form of k̄_i)
__global__ __launch_bounds__(256) void k_weighted_sum(long long n, double* __restrict__ out, WeightedSum ws) {
  const long long stride = (long long)gridDim.x * 256;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += stride) {
    double v = 0.0;
    for (int q = 0; q < ws.n; ++q) v += ws.w[q] * ws.p[q][t];
    out[t] = v;
  }
}

template <typename ADJ>
int adjoint_destroy(ADJ* adj) {
  if (!adj) return INS_OK;
  delete adj;
  return INS_OK;
}

// the checks that need no device, then the 2·nstage + 1 vector fields and one scalar of the isothermal step, zeroed
template <typename ADJ, typename T, typename PS>
int adjoint_create(const ins_grid* G, PS* ps, int nstage, const double* A, const double* c, ADJ** out, const char* name) {
  INS_REQUIRE(nstage >= 1 && nstage <= INS_MAX_STAGES, "unsupported number of stages");
  for (int i = 0; i < nstage; ++i)
    for (int j = i + 1; j < nstage; ++j) INS_REQUIRE(A[i * nstage + j] == 0.0, "shifted tableau must be lower triangular (explicit method)");
  for (int b = 0; b < G->g.D; ++b)
    if (G->g.bc[b][0] == INS_BC_HALO || G->g.bc[b][1] == INS_BC_HALO) {
      ins_set_error("%s: slab grids are not supported", name);
      return INS_ERR_UNSUPPORTED;
    }
  ADJ* adj = new ADJ();
  adj->grid = G;
  adj->ps = ps;
  adj->nstage = nstage;
  adj->A.assign(A, A + nstage * nstage);
  adj->c.assign(c, c + nstage);
  adj->v.resize(nstage);
  adj->y.resize(nstage);
  const size_t nvec = (size_t)G->ncell * G->g.D;
  int rc = adj->kbar.alloc_zero(nvec);
  if (rc == INS_OK) rc = adj->pwork.alloc_zero(G->ncell);
  for (int i = 0; rc == INS_OK && i < nstage; ++i)
    if ((rc = adj->v[i].alloc_zero(nvec)) == INS_OK) rc = adj->y[i].alloc_zero(nvec);
  if (rc != INS_OK) {
    adjoint_destroy(adj);
    return rc;
  }
  *out = adj;
  return INS_OK;
}

// the descriptor, and on its first arrival the 2·nstage + 1 scalar fields of the coupled step, zeroed
template <typename T, typename PS>
int adjoint_set_temperature(RkAdjointT<T, PS>* adj, const ins_temperature_desc_t* desc) {
  if (!desc) {
    adj->temp_on = false;
    return INS_OK;
  }
  const int D = adj->grid->g.D, ns = adj->nstage;
  INS_REQUIRE(desc->gdir >= 0 && desc->gdir < D, "gdir out of range");
  for (int q = 0; q < 2 * D; ++q)
    INS_REQUIRE(desc->bc[q] == INS_BC_PERIODIC || desc->bc[q] == INS_BC_DIRICHLET || desc->bc[q] == INS_BC_SYMMETRIC || desc->bc[q] == INS_BC_PRESSURE,
                "unsupported temperature boundary condition");
  const size_t ncell = (size_t)adj->grid->ncell;
  if (!adj->cbar) {
    adj->tau.clear(), adj->z.clear();
    adj->tau.resize(ns), adj->z.resize(ns);
    int rc = adj->cbar.alloc_zero(ncell);
    for (int i = 0; rc == INS_OK && i < ns; ++i)
      if ((rc = adj->tau[i].alloc_zero(ncell)) == INS_OK) rc = adj->z[i].alloc_zero(ncell);
    if (rc != INS_OK) {
      adj->tau.clear(), adj->z.clear(), adj->cbar.reset();
      return rc;
    }
  }
  adj->td = *desc;
  adj->temp_on = true;
  return INS_OK;
}

// kind, θ and the θ cotangent's address; on the first kind 1 the closure force's vector field and, where the force runs as three kernels, its `sigma`
// scratch, zeroed (the force writes degrees of freedom only)
template <typename T, typename PS>
int adjoint_set_closure(RkAdjointT<T, PS>* adj, int32_t kind, double theta, double* thetabar) {
  INS_REQUIRE(kind == 0 || kind == 1, "unknown closure kind");
  if (kind == 1 && !adj->mforce) {
    const ins_grid* G = adj->grid;
    const int D = G->g.D;
    const size_t vbytes = (size_t)G->ncell * D * sizeof(T), tbytes = (size_t)G->ncell * (D * (D + 1) / 2) * sizeof(T);
    const bool need_sigma = ins_smagorinsky_force_needs_sigma(G) != 0;
    int rc = adj->mforce.alloc_zero(vbytes / sizeof(T));
    if (rc == INS_OK && need_sigma) rc = adj->sigma.alloc_zero(tbytes / sizeof(T));
    if (rc != INS_OK) {
      adj->mforce.reset(), adj->sigma.reset();
      return rc;
    }
  }
  adj->closure_kind = kind;
  adj->theta = kind ? theta : 0.0;
  adj->thetabar = kind ? thetabar : nullptr;
  return INS_OK;
}

// ∂L/∂(u_out, temp_out) -> ∂L/∂(ustart, tempstart): the argument checks of the coupled entries, then the generic loop
template <typename T, typename PS>
int step_pullback_ext(RkAdjointT<T, PS>* adj, T visc, const T* ustart, const T* tempstart, const T* bodyforce, T dt, T* ubar, T* tempbar, void* stream) {
  INS_REQUIRE(adj && ustart && ubar, "null argument");
  INS_REQUIRE(adj->temp_on, "the coupled step pullback needs ins_rk_adjoint_set_temperature");
  INS_REQUIRE(tempstart && tempbar, "null temperature argument");
  INS_REQUIRE(ubar != ustart && tempbar != tempstart, "the step pullback cannot run in place (ubar aliases ustart or tempbar aliases tempstart)");
  INS_REQUIRE(ubar != tempstart && tempbar != ustart && ubar != tempbar && ustart != tempstart, "the step pullback's arguments alias one another");
  INS_REQUIRE(!bodyforce || (bodyforce != ubar && bodyforce != tempbar), "the body force aliases an output");
  return rkadj::step_pullback(adj, true, visc, ustart, tempstart, bodyforce, dt, ubar, tempbar, as_stream(stream));
}

}  // namespace

extern "C" int ins_rk_adjoint_destroy(ins_rk_adjoint_t* adj) { return adjoint_destroy(adj); }
extern "C" int ins_rk_adjoint_destroy_f32(ins_rk_adjoint32_t* adj) { return adjoint_destroy(adj); }

extern "C" int ins_rk_adjoint_create(const ins_grid_t* G, ins_poisson_t* ps, int nstage, const double* A, const double* c, ins_rk_adjoint_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  return adjoint_create<ins_rk_adjoint, double>(G, ps, nstage, A, c, out, "ins_rk_adjoint_create");
}

extern "C" int ins_rk_adjoint_create_f32(const ins_grid_t* G, ins_poisson32_t* ps, int nstage, const double* A, const double* c, ins_rk_adjoint32_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ins_k32_solver_grid(ps) == G, "psolver was created for a different grid");
  double* p64 = nullptr;
  const ins_poisson* ps64 = ins_k32_wrapped(ps, &p64);
  if (ps64 && ps64->kind == POISSON_SPECTRAL && G->all_periodic) {  // what ins_project_pullback_f32 refuses
    ins_set_error("ins_rk_adjoint_create_f32: a wrapped spectral solver on an all-periodic box is not taken (use ins_poisson_spectral_create_f32)");
    return INS_ERR_UNSUPPORTED;
  }
  return adjoint_create<ins_rk_adjoint32, float>(G, ps, nstage, A, c, out, "ins_rk_adjoint_create_f32");
}

extern "C" int ins_rk_adjoint_set_temperature(ins_rk_adjoint_t* adj, const ins_temperature_desc_t* desc) {
  INS_REQUIRE(adj, "null argument");
  return adjoint_set_temperature(adj, desc);
}

extern "C" int ins_rk_adjoint_set_temperature_f32(ins_rk_adjoint32_t* adj, const ins_temperature_desc_t* desc) {
  INS_REQUIRE(adj, "null argument");
  return adjoint_set_temperature(adj, desc);
}

extern "C" int ins_rk_adjoint_set_closure(ins_rk_adjoint_t* adj, int32_t kind, double theta, double* thetabar) {
  INS_REQUIRE(adj, "null argument");
  return adjoint_set_closure(adj, kind, theta, thetabar);
}

extern "C" int ins_rk_adjoint_set_closure_f32(ins_rk_adjoint32_t* adj, int32_t kind, double theta, double* thetabar) {
  INS_REQUIRE(adj, "null argument");
  return adjoint_set_closure(adj, kind, theta, thetabar);
}

extern "C" int ins_rk_step_pullback_f32(ins_rk_adjoint32_t* adj, float visc, const float* ustart, const float* bodyforce, float dt, float* ubar, void* stream) {
  INS_REQUIRE(adj && ustart && ubar, "null argument");
  INS_REQUIRE(ubar != ustart, "the step pullback cannot run in place (ubar aliases ustart)");
  INS_REQUIRE(!bodyforce || bodyforce != ubar, "the body force aliases the output");
  return rkadj::step_pullback<float, ins_poisson32>(adj, false, visc, ustart, nullptr, bodyforce, dt, ubar, nullptr, as_stream(stream));
}

extern "C" int ins_rk_step_pullback_ext_f64(ins_rk_adjoint_t* adj, double visc, const double* ustart, const double* tempstart, const double* bodyforce, double dt,
                                            double* ubar, double* tempbar, void* stream) {
  return step_pullback_ext<double, ins_poisson>(adj, visc, ustart, tempstart, bodyforce, dt, ubar, tempbar, stream);
}

extern "C" int ins_rk_step_pullback_ext_f32(ins_rk_adjoint32_t* adj, float visc, const float* ustart, const float* tempstart, const float* bodyforce, float dt,
                                            float* ubar, float* tempbar, void* stream) {
  return step_pullback_ext<float, ins_poisson32>(adj, visc, ustart, tempstart, bodyforce, dt, ubar, tempbar, stream);
}

extern "C" int ins_rk_step_pullback_f64(ins_rk_adjoint_t* adj, double visc, const double* ustart, const double* bodyforce, double dt, double* ubar,
                                        void* stream) {
  INS_REQUIRE(adj && ustart && ubar, "null argument");
  INS_REQUIRE(ubar != ustart, "the step pullback cannot run in place (ubar aliases ustart)");
  if (adj->closure_kind) {  // the closure lives in the generic loop
    INS_REQUIRE(!bodyforce || bodyforce != ubar, "the body force aliases the output");
    return rkadj::step_pullback<double, ins_poisson>(adj, false, visc, ustart, nullptr, bodyforce, dt, ubar, nullptr, as_stream(stream));
  }
  const ins_grid* G = adj->grid;
  hipStream_t s = as_stream(stream);
  const int ns = adj->nstage;
  const double* A = adj->A.data();
  const long long nvec = G->ncell * G->g.D;
  const size_t vbytes = (size_t)nvec * sizeof(double);
  int rc;

  // ---- the stage inputs v_i, k-basis, the kernel sequence of the reference (k_i lives in y[i] until the reverse sweep overwrites it)
  INS_HIP_TRY(hipMemcpyAsync(adj->v[0], ustart, vbytes, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < ns; ++i) {
    if ((rc = ins_k_apply_bc_u(G, adj->v[i], 0, nullptr, s))) return rc;  // :19
    if (i == ns - 1) break;                                               // the last k enters u_out only
    if ((rc = ins_k_momentum(G, visc, adj->v[i], adj->y[i], s))) return rc;  // :21
    double coef[INS_MAX_STAGES + 1];
    const double* k[INS_MAX_STAGES + 1];
    const int n = ins_rk_sum_terms(A, ns, i, dt, adj->y, bodyforce, coef, k);  // :35-38
    if ((rc = ins_combine_f64(G, ustart, adj->v[i + 1], n, coef, k, stream))) return rc;
    if ((rc = ins_k_apply_bc_u(G, adj->v[i + 1], 0, nullptr, s))) return rc;          // :48
    if ((rc = ins_k_project(G, adj->ps, adj->v[i + 1], adj->pwork, s))) return rc;    // :49
  }

  // ---- reverse sweep.  g lives in y[i] while it becomes ȳ_i; the pullback of stage i writes the next g into y[i-1], the last one into ubar,
  // whose own content has moved to y[ns-1] by then.
  const bool fused = ins_opt(OPT_INS_ADJ_STAGE_FUSED) != 0;
  INS_HIP_TRY(hipMemcpyAsync(adj->y[ns - 1], ubar, vbytes, hipMemcpyDeviceToDevice, s));
  for (int i = ns - 1; i >= 0; --i) {
    double* g = adj->y[i];
    if ((rc = ins_k_apply_bc_u_pullback(G, g, s))) return rc;                                 // :55 (i = ns-1) or :19 of stage i+1
    if ((rc = ins_project_pullback_f64(G, adj->ps, g, adj->pwork, stream))) return rc;        // :49
    if ((rc = ins_k_apply_bc_u_pullback(G, g, s))) return rc;                                 // :48
    WeightedSum ws;
    ws.n = 0;
    for (int ip = i; ip < ns; ++ip) {
      const double w = dt * A[ip * ns + i];
      if (w == 0.0) continue;
      ws.w[ws.n] = w;
      ws.p[ws.n] = adj->y[ip];
      ++ws.n;
    }
    double* out = i > 0 ? adj->y[i - 1] : ubar;
    if (ws.n == 0) {
      INS_HIP_TRY(hipMemsetAsync(out, 0, vbytes, s));
    } else if (fused && ws.n <= INS_ADJ_COMB_MAX) {
      if ((rc = ins_k_momentum_pullback_comb(G, visc, adj->v[i], ws.n, ws.w, ws.p, out, s))) return rc;
    } else {
      const unsigned nblk = (unsigned)std::min<long long>((nvec + 255) / 256, 8192);
      hipLaunchKernelGGL(k_weighted_sum, dim3(nblk), dim3(256), 0, s, nvec, adj->kbar, ws);
      INS_LAUNCH_CHECK();
      if ((rc = ins_momentum_pullback_f64(G, visc, adj->v[i], adj->kbar, out, 0, stream))) return rc;
    }
  }
  if ((rc = ins_k_apply_bc_u_pullback(G, ubar, s))) return rc;  // :19 of stage 0
  double one[INS_MAX_STAGES];
  const double* ybar[INS_MAX_STAGES];
  for (int i = 0; i < ns; ++i) one[i] = 1.0, ybar[i] = adj->y[i];
  return ins_combine_f64(G, ubar, ubar, ns, one, ybar, stream);
}
