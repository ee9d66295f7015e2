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
#include "ins_adjoint_kernels.h"
#include "ins_rk_terms.h"

int ins_k_apply_bc_u_pullback(const ins_grid* G, double* u, hipStream_t s);
int ins_k_momentum_pullback_comb(const ins_grid* G, double visc, const double* u, int nterms, const double* coefs, const double* const* ks, double* ubar,
                                 hipStream_t s);

struct ins_rk_adjoint {
  const ins_grid* grid = nullptr;
  ins_poisson* ps = nullptr;
  int nstage = 0;
  std::vector<double> A, c;
  std::vector<double*> v;  // stage inputs v_i (ghosts filled)
  std::vector<double*> y;  // k_i during the recomputation, then the stage cotangents ȳ_i
  double* kbar = nullptr;
  double* pwork = nullptr;
};

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

}  // namespace

extern "C" int ins_rk_adjoint_destroy(ins_rk_adjoint_t* adj) {
  if (!adj) return INS_OK;
  for (double* p : adj->v)
    if (p) (void)hipFree(p);
  for (double* p : adj->y)
    if (p) (void)hipFree(p);
  if (adj->kbar) (void)hipFree(adj->kbar);
  if (adj->pwork) (void)hipFree(adj->pwork);
  delete adj;
  return INS_OK;
}

extern "C" int ins_rk_adjoint_create(const ins_grid_t* G, ins_poisson_t* ps, int nstage, const double* A, const double* c, ins_rk_adjoint_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  INS_REQUIRE(nstage >= 1 && nstage <= INS_MAX_STAGES, "unsupported number of stages");
  for (int i = 0; i < nstage; ++i)
    for (int j = i + 1; j < nstage; ++j) INS_REQUIRE(A[i * nstage + j] == 0.0, "shifted tableau must be lower triangular (explicit method)");
  for (int b = 0; b < G->g.D; ++b)
    if (G->g.bc[b][0] == INS_BC_HALO || G->g.bc[b][1] == INS_BC_HALO) {
      ins_set_error("ins_rk_adjoint_create: slab grids are not supported");
      return INS_ERR_UNSUPPORTED;
    }
  ins_rk_adjoint* adj = new ins_rk_adjoint();
  adj->grid = G;
  adj->ps = ps;
  adj->nstage = nstage;
  adj->A.assign(A, A + nstage * nstage);
  adj->c.assign(c, c + nstage);
  adj->v.assign(nstage, nullptr);
  adj->y.assign(nstage, nullptr);
  const size_t vbytes = (size_t)G->ncell * G->g.D * sizeof(double), sbytes = (size_t)G->ncell * sizeof(double);
  bool ok = hipMalloc(&adj->kbar, vbytes) == hipSuccess && hipMalloc(&adj->pwork, sbytes) == hipSuccess;
  for (int i = 0; ok && i < nstage; ++i) ok = hipMalloc(&adj->v[i], vbytes) == hipSuccess && hipMalloc(&adj->y[i], vbytes) == hipSuccess;
  if (ok) ok = hipMemset(adj->pwork, 0, sbytes) == hipSuccess && hipMemset(adj->kbar, 0, vbytes) == hipSuccess;
  for (int i = 0; ok && i < nstage; ++i) ok = hipMemset(adj->v[i], 0, vbytes) == hipSuccess && hipMemset(adj->y[i], 0, vbytes) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    ins_set_error("ins_rk_adjoint_create: device allocation of %d vector fields failed", 2 * nstage + 1);
    ins_rk_adjoint_destroy(adj);
    return INS_ERR_HIP;
  }
  *out = adj;
  return INS_OK;
}

extern "C" int ins_rk_step_pullback_f64(ins_rk_adjoint_t* adj, double visc, const double* ustart, const double* bodyforce, double dt, double* ubar,
                                        void* stream) {
  INS_REQUIRE(adj && ustart && ubar, "null argument");
  INS_REQUIRE(ubar != ustart, "the step pullback cannot run in place (ubar aliases ustart)");
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
    const int n = ins_rk_sum_terms(A, ns, i, dt, adj->y.data(), bodyforce, coef, k);  // :35-38
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
  for (int i = 0; i < ns; ++i) one[i] = 1.0;
  return ins_combine_f64(G, ubar, ubar, ns, one, adj->y.data(), stream);
}
