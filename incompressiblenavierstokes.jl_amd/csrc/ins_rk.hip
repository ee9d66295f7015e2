// Explicit Runge-Kutta stage loop (step_explicit_runge_kutta.jl:4-59) and its cache
// (time_stepper_caches.jl:34-49).
#include <cstdlib>

#include "ins_debug.h"
#include "ins_internal.h"
#include "ins_rk_terms.h"

int ins_k_momentum(const ins_grid* G, double visc, const double* u, double* F, hipStream_t s) {
  if (ins_fast3d_supported(G)) return ins_k_momentum_fast3d(G, visc, u, F, s);
  return ins_k_momentum_generic(G, visc, u, F, s);
}

namespace {

struct Combine {
  int n;
  double coef[INS_MAX_STAGES + 1];  // + 1: the steady body force is one more term (ins_rk_set_bodyforce)
  const double* k[INS_MAX_STAGES + 1];
};

// K6: u = ustart + Σ_j (Δt A[i,j]) ku[j]  in ONE pass (the reference does 1 copy + i axpy passes and does
// not skip tableau zeros, step_explicit_runge_kutta.jl:35-38).  Summation order as in the reference.
__global__ __launch_bounds__(256) void k_combine(long long n, const double* ustart, double* u, Combine cb) {
  const long long stride = (long long)gridDim.x * 256 * 2;
  for (long long t = ((long long)blockIdx.x * 256 + threadIdx.x) * 2; t < n; t += stride) {
    if (t + 1 < n) {
      double2 v = *reinterpret_cast<const double2*>(ustart + t);
      for (int j = 0; j < cb.n; ++j) {
        const double2 kv = *reinterpret_cast<const double2*>(cb.k[j] + t);
        v.x += cb.coef[j] * kv.x;
        v.y += cb.coef[j] * kv.y;
      }
      *reinterpret_cast<double2*>(u + t) = v;
    } else {
      double v = ustart[t];
      for (int j = 0; j < cb.n; ++j) v += cb.coef[j] * cb.k[j][t];
      u[t] = v;
    }
  }
}

}  // namespace

static int combine_n(long long nvec, const double* base, double* out, int nterms, const double* coefs, const double* const* ks, void* stream);

extern "C" int ins_combine_f64(const ins_grid_t* G, const double* base, double* out, int nterms, const double* coefs,
                               const double* const* ks, void* stream) {
  INS_REQUIRE(G && base && out, "null argument");
  return combine_n(G->ncell * G->g.D, base, out, nterms, coefs, ks, stream);
}

extern "C" int ins_combine_scalar_f64(const ins_grid_t* G, const double* base, double* out, int nterms, const double* coefs,
                                      const double* const* ks, void* stream) {
  INS_REQUIRE(G && base && out, "null argument");
  return combine_n(G->ncell, base, out, nterms, coefs, ks, stream);
}

static int combine_n(long long nvec, const double* base, double* out, int nterms, const double* coefs, const double* const* ks, void* stream) {
  INS_REQUIRE(nterms >= 0 && nterms <= INS_MAX_STAGES + 1 && (nterms == 0 || (coefs && ks)), "bad stage terms");
  Combine cb;
  cb.n = 0;
  for (int q = 0; q < nterms; ++q) {
    if (coefs[q] == 0.0) continue;
    INS_REQUIRE(ks[q], "null stage field");
    cb.coef[cb.n] = coefs[q];
    cb.k[cb.n] = ks[q];
    ++cb.n;
  }
  const unsigned nblk = (unsigned)std::min<long long>((nvec / 2 + 255) / 256, 8192);
  hipLaunchKernelGGL(k_combine, dim3(nblk), dim3(256), 0, as_stream(stream), nvec, base, out, cb);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

static void step_graph_free(ins_rk* rk);

extern "C" int ins_rk_create(const ins_grid_t* G, ins_poisson_t* ps, int nstage, const double* A, const double* c, ins_rk_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  INS_REQUIRE(nstage >= 1 && nstage <= INS_MAX_STAGES, "unsupported number of stages");
  for (int i = 0; i < nstage; ++i)
    for (int j = i + 1; j < nstage; ++j) INS_REQUIRE(A[i * nstage + j] == 0.0, "shifted tableau must be lower triangular (explicit method)");
  ins_rk* rk = new ins_rk();
  rk->grid = G;
  rk->ps = ps;
  rk->nstage = nstage;
  rk->A.assign(A, A + nstage * nstage);
  rk->c.assign(c, c + nstage);
  const size_t nvec = (size_t)G->ncell * G->g.D;
  rk->ku.resize(nstage);
  int rc = rk->ustart.alloc_zero(nvec);
  if (rc == INS_OK) rc = rk->p.alloc_zero(G->ncell);
  for (int i = 0; rc == INS_OK && i < nstage; ++i) rc = rk->ku[i].alloc_zero(nvec);
  if (rc != INS_OK) {
    ins_rk_destroy(rk);
    return rc;
  }
  *out = rk;
  return INS_OK;
}

extern "C" int ins_rk_destroy(ins_rk_t* rk) {
  if (!rk) return INS_OK;
  for (hipEvent_t e : rk->prof_events) (void)hipEventDestroy(e);
  ins_rk_ext_free(rk->ext);
  step_graph_free(rk);
  delete rk;
  return INS_OK;
}

extern "C" int ins_rk_profile_enable(ins_rk_t* rk, int enable) {
  INS_REQUIRE(rk, "null argument");
  rk->profiling = enable != 0;
  return INS_OK;
}

extern "C" int ins_rk_profile_read(ins_rk_t* rk, double* momentum_ms, int64_t* momentum_launches) {
  INS_REQUIRE(rk && momentum_ms && momentum_launches, "null argument");
  double total = 0.0;
  const size_t n = rk->prof_events.size() / 2;
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    INS_HIP_TRY(hipEventSynchronize(rk->prof_events[2 * i + 1]));
    INS_HIP_TRY(hipEventElapsedTime(&ms, rk->prof_events[2 * i], rk->prof_events[2 * i + 1]));
    total += ms;
  }
  for (hipEvent_t e : rk->prof_events) (void)hipEventDestroy(e);
  rk->prof_events.clear();
  *momentum_ms = total;
  *momentum_launches = (int64_t)n;
  return INS_OK;
}

extern "C" int ins_rk_pressure(const ins_rk_t* rk, double** p) {
  INS_REQUIRE(rk && p, "null argument");
  *p = rk->p;
  return INS_OK;
}

// How many stage kernels of this integrator have written the Poisson right-hand side themselves so far (a test asserts that the route ran).
extern "C" int ins_dbg_stage_rhs_used(const ins_rk_t* rk, int64_t* launches) {
  INS_REQUIRE(rk && launches, "null argument");
  *launches = (int64_t)rk->stage_rhs_launches;
  return INS_OK;
}

// How many of them stored the x-spectrum of the right-hand side instead of the real-space array (ins_flux64.hip, XF).
extern "C" int ins_dbg_stage_xfwd_used(const ins_rk_t* rk, int64_t* launches) {
  INS_REQUIRE(rk && launches, "null argument");
  *launches = (int64_t)rk->stage_xfwd_launches;
  return INS_OK;
}

// How many stage kernels of this integrator have stored a carried combination so far (RkCarryPlan, ins_rk_terms.h; a test asserts that the route ran).
extern "C" int ins_dbg_stage_carry_used(const ins_rk_t* rk, int64_t* launches) {
  INS_REQUIRE(rk && launches, "null argument");
  *launches = (int64_t)rk->stage_carry_launches;
  return INS_OK;
}

// Test hook (needs no device): the carry plan of the caller's tableau.  *j < 0: no plan.  With a plan: a[3], and the consuming stage's terms as
// ins_rk_carry_consumer_terms builds them: *self_in, *coef_self and *coef_force (0 without a force); it starts from S with factor 1.
extern "C" int ins_dbg_rk_carry_plan(int32_t ns, const double* A, double dt, int32_t with_force, int32_t* j, int32_t* i, double* a, double* self_in,
                                     double* coef_self, double* coef_force) {
  INS_REQUIRE(A && j && i && a && self_in && coef_self && coef_force, "null argument");
  INS_REQUIRE(ns >= 1 && ns <= INS_MAX_STAGES, "bad argument");
  const RkCarryPlan pl = ins_rk_carry_plan(A, ns);
  *j = pl.j, *i = pl.i, *self_in = 0.0, *coef_self = 0.0, *coef_force = 0.0;
  for (int q = 0; q < 3; ++q) a[q] = pl.a[q];
  if (pl.j < 0) return INS_OK;
  static double slot[2];
  const RkEpi epi = ins_rk_carry_consumer_terms<double>(A, ns, pl, dt, slot, with_force ? slot + 1 : nullptr);
  INS_REQUIRE(epi.ustart == slot && epi.c0m1 == 0.0 && epi.n == (with_force ? 1 : 0), "consumer terms");
  *self_in = epi.self_in, *coef_self = epi.coef_self;
  if (with_force) *coef_force = epi.coef[0];
  return INS_OK;
}

// Test hook: ONE stage kernel through the production dispatch, u* = (1 - self_in) ustart + self_in u_in + coef_k kterm + coef_self F(u_in), stored to ustar
// (interior volumes), with Ω·div(u*) copied to rhs (unpadded n^3, device) where the stage kernel writes it; *used says whether it did.  pI == nullptr: u_in
// has valid ghost volumes; else u_in is an uncorrected stage velocity and pI its unpadded pressure (the in-register correction).  ustart / kterm nullable.
extern "C" int ins_dbg_stage_rhs(ins_rk_t* rk, double visc, const double* u_in, const double* pI, const double* ustart, const double* kterm, double coef_k,
                                 double self_in, double coef_self, double* ustar, double* rhs, int32_t* used, void* stream) {
  INS_REQUIRE(rk && u_in && ustar && rhs && used, "null argument");
  const ins_grid* G = rk->grid;
  hipStream_t s = as_stream(stream);
  RkEpi epi;
  memset(&epi, 0, sizeof(epi));
  epi.ustart = ustart;
  epi.ustar = ustar;
  epi.coef_self = coef_self;
  if (ustart) {
    epi.self_in = self_in;
    epi.c0m1 = -self_in;
  }
  if (kterm) {
    epi.coef[0] = coef_k;
    epi.k[0] = kterm;
    epi.n = 1;
  }
  *used = 0;
  INS_REQUIRE(!ins_stage_out_aliases_input(epi, u_in), "ustar must be an array of its own");
  if (ins_flux64_stage_rhs_supported(G, pI ? 1 : 0) && (epi.rhs_out = ins_poisson_stage_rhs(rk->ps))) *used = 1;
  int rc = pI ? ins_k_momentum_rk_fused_corr(G, visc, u_in, pI, rk->ku[0], epi, s) : ins_k_momentum_rk_fused(G, visc, u_in, rk->ku[0], epi, s);
  if (rc) return rc;
  if (*used) INS_HIP_TRY(hipMemcpyAsync(rhs, epi.rhs_out, (size_t)rk->ps->np[0] * rk->ps->np[1] * rk->ps->np[2] * sizeof(double), hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

// Test hook: the same launch on the x-spectrum route.  The stage kernel stores the half-complex x-spectrum of Ω·div(u*) into the solver's spectrum buffer, which is
// copied to spec (n2 · n1 · kxs complex numbers, kxs = n0/2 + 1 rounded up to 8; device); *used says whether the route was taken (else nothing is launched).
extern "C" int ins_dbg_stage_xfwd(ins_rk_t* rk, double visc, const double* u_in, const double* pI, const double* ustart, const double* kterm, double coef_k,
                                  double self_in, double coef_self, double* ustar, double* spec, int32_t* used, void* stream) {
  INS_REQUIRE(rk && u_in && ustar && spec && used, "null argument");
  const ins_grid* G = rk->grid;
  hipStream_t s = as_stream(stream);
  RkEpi epi;
  memset(&epi, 0, sizeof(epi));
  epi.ustart = ustart;
  epi.ustar = ustar;
  epi.coef_self = coef_self;
  if (ustart) {
    epi.self_in = self_in;
    epi.c0m1 = -self_in;
  }
  if (kterm) {
    epi.coef[0] = coef_k;
    epi.k[0] = kterm;
    epi.n = 1;
  }
  *used = 0;
  INS_REQUIRE(!ins_stage_out_aliases_input(epi, u_in), "ustar must be an array of its own");
  if (!pI || !ins_flux64_stage_xfwd_supported(G, 1) || !(epi.spec_out = ins_poisson_stage_spec(rk->ps, pI, &epi.spec_tw, &epi.spec_kxs))) return INS_OK;
  rk->ps->spec_pending = false;  // (no solve follows: the buffer is only read back)
  *used = 1;
  int rc = ins_k_momentum_rk_fused_corr(G, visc, u_in, pI, rk->ku[0], epi, s);
  if (rc) return rc;
  INS_HIP_TRY(hipMemcpyAsync(spec, epi.spec_out, (size_t)epi.spec_kxs * rk->ps->np[1] * rk->ps->np[2] * 2 * sizeof(double), hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

// Test hook (tests/test_rk_stage_terms.py; needs no device): the builders of ins_rk_terms.h on the caller's tableau.  kind 0 / 1: ins_rk_stage_terms in
// the k-basis / the stage-velocity basis (order 0: force sum diagonal first, 1: index order); kind 2 / 3: ins_rk_sum_terms in double / float.
// stage[q], coef[q] (room for INS_MAX_STAGES + 1): earlier stage and coefficient of term q; the force term reports stage ns and its coefficient also in
// *coef_force (0 without a force).
extern "C" int ins_dbg_rk_stage_terms(int32_t ns, const double* A, int32_t i, double dt, int32_t kind, int32_t input_in_regs, int32_t with_force, int32_t order,
                                      int32_t* n, int32_t* stage, double* coef, double* c0m1, double* self_in, double* coef_self, int32_t* write_k,
                                      double* coef_force) {
  INS_REQUIRE(A && n && stage && coef && c0m1 && self_in && coef_self && write_k && coef_force, "null argument");
  INS_REQUIRE(ns >= 1 && ns <= INS_MAX_STAGES && i >= 0 && i < ns && kind >= 0 && kind <= 3, "bad argument");
  INS_REQUIRE(kind != 1 || ins_rk_vbasis_possible(A, ns), "the stage-velocity basis needs a non-zero diagonal");
  static double slot[INS_MAX_STAGES + 1];  // stands for the stage arrays: term q's stage is k[q] - slot
  double* prev[INS_MAX_STAGES];
  for (int m = 0; m < ns; ++m) prev[m] = slot + m;
  const double* force = with_force ? slot + ns : nullptr;
  RkEpi epi;
  memset(&epi, 0, sizeof(epi));
  if (kind <= 1) {
    epi = ins_rk_stage_terms(A, ns, i, dt, prev, force, kind ? RK_V_BASIS : RK_K_BASIS, input_in_regs != 0, order ? RK_FORCE_INDEX_ORDER : RK_FORCE_DIAG_FIRST);
  } else if (kind == 2) {
    epi.n = ins_rk_sum_terms(A, ns, i, dt, prev, force, epi.coef, epi.k);
  } else {
    float cf32[INS_MAX_STAGES + 1];
    epi.n = ins_rk_sum_terms(A, ns, i, (float)dt, prev, force, cf32, epi.k);
    for (int q = 0; q < epi.n; ++q) epi.coef[q] = cf32[q];
  }
  *n = epi.n, *c0m1 = epi.c0m1, *self_in = epi.self_in, *coef_self = epi.coef_self, *write_k = epi.write_k, *coef_force = 0.0;
  for (int q = 0; q < epi.n; ++q) {
    stage[q] = (int32_t)(epi.k[q] - slot);
    coef[q] = epi.coef[q];
    if (epi.k[q] == force) *coef_force = epi.coef[q];
  }
  return INS_OK;
}

extern "C" int ins_rk_set_bodyforce(ins_rk_t* rk, const double* force) {
  INS_REQUIRE(rk, "null argument");
  rk->force = force;
  return INS_OK;
}

extern "C" int ins_rk_stage_force(const ins_rk_t* rk, int i, double** ku) {
  INS_REQUIRE(rk && ku, "null argument");
  INS_REQUIRE(i >= 0 && i < rk->nstage, "stage index out of range");
  *ku = rk->ku[i];
  return INS_OK;
}

// rk->profiling: an event pair on the stream around the stage kernel that `launch` enqueues (ins_rk_profile_read); kept only when the launch succeeded
template <typename F>
static int timed_stage(ins_rk* rk, hipStream_t s, F&& launch) {
  if (!rk->profiling) return launch();
  hipEvent_t e0 = nullptr, e1 = nullptr;
  INS_HIP_TRY(hipEventCreate(&e0));
  INS_HIP_TRY(hipEventCreate(&e1));
  INS_HIP_TRY(hipEventRecord(e0, s));
  const int rc = launch();
  if (rc) return rc;
  INS_HIP_TRY(hipEventRecord(e1, s));
  rk->prof_events.push_back(e0);
  rk->prof_events.push_back(e1);
  return INS_OK;
}

// The two ping-pong stage buffers, allocated on first use.  The periodic loops zero them (init_from == nullptr); the tiled loops copy the caller's
// field into them once: volumes no kernel ever writes.
int ins_rk_ensure_ub(ins_rk* rk, size_t bytes, hipStream_t s, const double* init_from) {
  for (int b = 0; b < 2; ++b)
    if (!rk->ub[b]) {
      const size_t n = bytes / sizeof(double);
      if (int rc = init_from ? rk->ub[b].alloc_copy_device(n, init_from, s) : rk->ub[b].alloc_zero_async(n, s)) return rc;
    }
  return INS_OK;
}

// Fused periodic path (3-D, all-periodic, spectral solver): per stage
//   K1+K6  k_i = momentum(u_in), u* = ustart + Σ Δt a_ij k_j      (one pass; u* goes to a ping-pong buffer)
//   K2     pI = Ω div(u*) with periodic wrap                      (no ghost fill of u* needed)
//   rocFFT forward, K3 symbol, rocFFT inverse
//   K4     u* -= ∇p on the interior + its periodic ghost images    (no apply_bc_u! launch)
// Same arithmetic, in the same order, as the reference stage loop (step_explicit_runge_kutta.jl:17-50);
// `ustart` is the caller's `u`, which stays untouched until the last stage writes the result into it.
// chain: 0 = a whole step (u valid in, valid out); bit 1 = `u` holds the previous step's UNCORRECTED result and ps->pI its pressure
// (the first stage corrects in registers and stores the corrected field as ustart); bit 2 = leave this step's result uncorrected in `u`.
static int rk_step_fused_periodic(ins_rk* rk, double visc, double* u, double dt, hipStream_t s, int chain = 0) {
  const ins_grid* G = rk->grid;
  const int ns = rk->nstage;
  const size_t vbytes = (size_t)G->ncell * 3 * sizeof(double);
  int rc;
  if ((rc = ins_rk_ensure_ub(rk, vbytes, s, nullptr))) return rc;
  const bool raw_in = chain & 1, raw_out = chain & 2;
  if (!raw_in && (rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;  // :19 (first stage; later ghosts come from K4)
  // On exactly-uniform grids stages >= 2 read the previous stage's UNCORRECTED u* plus its pressure and apply
  // the projection's gradient-subtract in registers (k_momentum_flux<..., CORR>), so K4 runs for the last stage only.
  const bool inkernel = ins_rk_inkernel3d(rk);
  // Stage-velocity basis (ins_rk_terms.h): with the in-kernel correction no k_j is written or read.  INS_RK_KEEP_K=1 restores the k-basis (and fills the
  // ku cache arrays, which this basis leaves untouched).
  const bool vbasis = inkernel && !ins_opt(OPT_INS_RK_KEEP_K) && ins_rk_vbasis_possible(rk->A.data(), ns);
  if (vbasis && (int)rk->vb.size() < ns - 1) {
    rk->vb.resize(ns - 1, nullptr);
    for (int m = 0; m < ns - 1; ++m)
      if (!rk->vb[m]) {
        if (m < 2 && rk->ub[m]) {
          rk->vb[m] = rk->ub[m];
          continue;
        }
        rk->vb_extra.emplace_back();
        if (int rc2 = rk->vb_extra.back().alloc_zero_async(vbytes / sizeof(double), s)) return rc2;
        rk->vb[m] = rk->vb_extra.back();
      }
  }
  // Carry plan (ins_rk_terms.h; INS_DISABLE_STAGE_CARRY=1 switches it off): stage pl.j also stores S, the part of the last stage's combination it has in
  // registers, and the last stage starts from S instead of loading ustart, V_{j-1} and V_j.  Where the 64-wide correcting kernel runs stage pl.j only.
  // Buffers (rk->vb is private to this loop, the pointers are the same in every step): S takes vb[j+1], which nothing uses before stage j+1 stores into it;
  // stage j+1 stores V_{j+1} to vb[j-1] instead (V_{j-1} is dead once stage j has finished, and stage j+1 reads no cell of it).  Never S to vb[j-1] during
  // stage j: other workgroups still read V_{j-1}'s halo rows and planes.
  RkCarryPlan pl = {-1, -1, {0.0, 0.0, 0.0}};
  if (vbasis && ins_flux64_stage_carry_supported(G)) pl = ins_rk_carry_plan(rk->A.data(), ns);
  const bool carry = pl.j >= 0;
  const double* in = u;
  double* tab[INS_MAX_STAGES];  // the arrays of the earlier stages in this basis: V_m or k_m
  for (int m = 0; m < ns - 1; ++m) tab[m] = vbasis ? rk->vb[m] : rk->ku[m].get();
  for (int i = 0; i < ns; ++i) {
    double* out = (i == ns - 1 && ns > 1) ? u : (vbasis ? rk->vb[(carry && i == pl.j + 1) ? pl.j - 1 : i] : rk->ub[i & 1]);
    // the V_m live in rk->vb; V_{i-1}, the stencil input, comes from registers on the 64-wide kernel only (the 62-wide one keeps no uncorrected copy)
    RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, dt, tab, rk->force, vbasis ? RK_V_BASIS : RK_K_BASIS,
                                   vbasis && ins_flux64_supported(G), RK_FORCE_DIAG_FIRST);
    epi.ustart = (i == 0) ? nullptr : (raw_in ? rk->ustart : u);  // raw_in: the corrected start field lives in the cache array
    epi.ustar = out;
    // the last stage of a step that is not chained to its predecessor stores u* over the caller's u, its ustart, and keeps the old right-hand-side route for that;
    // with the plan it no longer reads u, but which stages write the right-hand side does not depend on the plan
    const bool in_place = ins_stage_out_aliases_input(epi, in);
    if (carry && i == pl.j) {
      epi.carry_out = rk->vb[pl.j + 1];
      for (int q = 0; q < 3; ++q) epi.ca[q] = pl.a[q];
      if (ins_stage_carry_aliases(epi, in) || in_place) {
        ins_set_error("carried stage combination: an output of stage %d is one of its inputs", i);
        return INS_ERR_INVALID;
      }
      ++rk->stage_carry_launches;
    }
    if (carry && i == pl.i) {
      epi = ins_rk_carry_consumer_terms(rk->A.data(), ns, pl, dt, rk->vb[pl.j + 1], rk->force);
      epi.ustar = out;
    }
    if (i == 0 && raw_in) epi.ustart_out = rk->ustart;
    // Where the stage kernel spans whole rows it also writes Ω·div(u*), and the solver's x pass reads that one array instead of the three components
    // of u* (INS_DISABLE_STAGE_RHS=1: the x pass forms it).  A buffer of its own: pI is the correcting kernel's pressure input.
    // Not where u* overwrites one of the kernel's inputs (the last stage of an unchained step: ustart == out == the caller's u): that is safe cell by cell,
    // but for the right-hand side a wavefront reads its neighbours' cells of the inputs (row jb0-1, plane k0-1), which another workgroup may have overwritten.
    const bool corr = inkernel && (i > 0 || raw_in);
    // 256-wide rows: it stores the x-forward transform of that right-hand side into the solver's spectrum buffer instead, and the solve starts at its y pass
    // (INS_DISABLE_STAGE_XFWD=1: the real-space array and the x pass again).  One predicate decides (ins_flux64_stage_xfwd_supported).
    if (!in_place && ins_flux64_stage_rhs_supported(G, corr ? 1 : 0)) {
      if (ins_flux64_stage_xfwd_supported(G, corr ? 1 : 0) && ins_poisson_stage_spec_possible(rk->ps) &&
          (epi.spec_out = ins_poisson_stage_spec(rk->ps, corr ? rk->ps->pI : nullptr, &epi.spec_tw, &epi.spec_kxs))) {
        ++rk->stage_rhs_launches;
        ++rk->stage_xfwd_launches;
      } else if ((epi.rhs_out = ins_poisson_stage_rhs(rk->ps))) {
        ++rk->stage_rhs_launches;
      }
    }
    rc = timed_stage(rk, s, [&] {
      return corr ? ins_k_momentum_rk_fused_corr(G, visc, in, rk->ps->pI, rk->ku[i], epi, s) : ins_k_momentum_rk_fused(G, visc, in, rk->ku[i], epi, s);
    });
    if (rc) return rc;
    rc = (inkernel && (i < ns - 1 || raw_out)) ? ins_k_project_periodic_solve_only(G, rk->ps, out, s, epi.rhs_out, epi.spec_out != nullptr)
                                               : ins_k_project_periodic_fused(G, rk->ps, out, rk->p, i == ns - 1, s, nullptr, epi.rhs_out, epi.spec_out != nullptr);
    if (rc) return rc;
    in = out;
  }
  if (ns == 1) INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], vbytes, hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

// Fused periodic path in 2-D (uniform periodic power-of-two boxes): per stage the flux-form stage kernel (K1 + K6, ins_flux2d.hip) and the
// four-launch projection above — five launches per stage instead of ten, which is what a 128² .. 512² grid is bound by; with the in-register correction
// (stages >= 2, ins_flux2d.hip CORR) the projections between two stages only solve: four launches per stage, 17 per RK44 step.
// chain: as rk_step_fused_periodic (bit 1: `u` holds the previous step's uncorrected result and ps->pI its pressure; bit 2: leave this step's result uncorrected).
static int rk_step_fused_periodic_2d(ins_rk* rk, double visc, double* u, double dt, hipStream_t s, int chain = 0) {
  const ins_grid* G = rk->grid;
  const int ns = rk->nstage;
  const size_t vbytes = (size_t)G->ncell * 2 * sizeof(double);
  int rc;
  if ((rc = ins_rk_ensure_ub(rk, vbytes, s, nullptr))) return rc;
  const bool raw_in = chain & 1, raw_out = chain & 2;
  if (!raw_in && (rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;  // :19 (first stage; later ghosts come with the gradient-subtract)
  const bool incorr = ins_rk_inkernel2d(rk);
  if (chain && !incorr) {
    ins_set_error("chained 2-D steps need the in-register correction");
    return INS_ERR_INVALID;
  }
  const double* in = u;
  for (int i = 0; i < ns; ++i) {
    double* out = (i == ns - 1 && ns > 1) ? u : rk->ub[i & 1];
    RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, RK_K_BASIS, false, RK_FORCE_INDEX_ORDER);  // k-basis only
    epi.ustart = (i == 0) ? nullptr : (raw_in ? rk->ustart : u);  // raw_in: the corrected start field lives in the cache array
    epi.ustar = out;
    if (i == 0 && raw_in) epi.ustart_out = rk->ustart;
    // stages >= 2 read the previous stage's UNCORRECTED u* and its pressure and correct in registers (k_flux2d<…, CORR>): between two stages the projection
    // only solves (three launches instead of four, 48 B per volume less); the last stage's projection materialises u, p and their ghosts
    rc = timed_stage(rk, s, [&] { return ins_k_flux2d(G, visc, in, rk->ku[i], &epi, s, (incorr && (i > 0 || raw_in)) ? rk->ps->pI : nullptr); });
    if (rc) return rc;
    rc = (incorr && (i < ns - 1 || raw_out)) ? ins_k_project_periodic_solve_only_2d(G, rk->ps, out, s) : ins_k_project_periodic_fused_2d(G, rk->ps, out, rk->p, i == ns - 1, s);
    if (rc) return rc;
    in = out;
  }
  if (ns == 1) INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], vbytes, hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------ a step as a hipGraph (opt-in: INS_STEP_GRAPH=1)
// A 32^3 .. 64^3 box (or a 2-D grid) runs ~24 dependent launches of a few microseconds each per RK44 step.  With INS_STEP_GRAPH=1 ins_rk_steps_f64 captures
// the launches of ONE step of its loop into a hipGraph the first time it sees (u, Δt, ν) and replays it for the following steps — the same kernels with the
// same arguments in the same order, so results are bitwise those of the plain loop (tests/test_gpu_step_graph.py).
// Measured (profiles/r03_step_graph_lab.txt, RK44): the HOST time to issue a step drops 0.09 -> 0.02 ms, but the device span GROWS — 32^3: 0.137 -> 0.168
// ms/step, 128^2: 0.113 -> 0.140 — because these steps are bound by the device's dependent-dispatch latency (~5.7 us per kernel), not by the host's issue
// rate, and a graph node costs ~1.2 us more than a stream launch on this runtime.  So the graph is NOT the default: it is for callers whose host thread has
// other work to do while the steps run (the reference's processors / a training loop), and the lever for small boxes is fewer launches per stage.
//   * all-periodic boxes on the spectral solver's own FFT passes only (no rocFFT / rocBLAS call, no host read inside the step);
//   * the caller's stream may be the legacy null stream, which cannot be captured: capture and replay run on a stream of the cache, ordered against
//     the caller's stream by events on both sides;
//   * the first step of a call always runs directly (lazy allocations and attribute settings happen there, none during the capture); a capture that fails
//     for any reason is dropped and the loop continues with direct launches.
struct StepGraph {
  hipStream_t gs = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr;
  hipGraphExec_t exec = nullptr;
  double* u = nullptr;
  double dt = 0.0, visc = 0.0;
  const double* force = nullptr;
  int kind = 0;
  long long epoch = -1;
  long long replays = 0;
  bool broken = false;  // a capture failed on this cache: do not try again
};

static void step_graph_free(ins_rk* rk) {
  StepGraph* g = static_cast<StepGraph*>(rk->step_graph);
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->ev_in) (void)hipEventDestroy(g->ev_in);
  if (g->ev_out) (void)hipEventDestroy(g->ev_out);
  if (g->gs) (void)hipStreamDestroy(g->gs);
  delete g;
  rk->step_graph = nullptr;
}

// test / lab hook: how many steps this cache has run as graph replays
extern "C" long long ins_dbg_rk_graph_replays(const ins_rk_t* rk) { return (rk && rk->step_graph) ? static_cast<const StepGraph*>(rk->step_graph)->replays : 0; }

// kind 1: the chained middle step of the fused periodic 3-D loop; 2: a whole fused periodic step (3-D without the chain, or 2-D).  0: no graph.
static int step_graph_kind(const ins_rk* rk, bool chain_ok) {
  const ins_grid* G = rk->grid;
  if (!ins_opt(OPT_INS_STEP_GRAPH) || ins_opt(OPT_INS_DISABLE_STEP_GRAPH) || rk->profiling || rk->ext) return 0;
  const bool own = G->g.D == 3 ? ins_rk_fused3d(rk) && ins_k_spectral_own3d(rk->ps) : ins_rk_fused2d(rk);
  return own ? (chain_ok ? 1 : 2) : 0;
}

// one step of the chained loop (3-D or 2-D fused periodic path)
static int chain_step(ins_rk* rk, double visc, double* u, double dt, hipStream_t s, int chain) {
  return rk->grid->g.D == 2 ? rk_step_fused_periodic_2d(rk, visc, u, dt, s, chain) : rk_step_fused_periodic(rk, visc, u, dt, s, chain);
}

// Capture `enqueue(gs)` into g->exec.  Nothing executes here.  false: no graph (the cache is marked broken).
template <typename F>
static bool step_graph_capture(StepGraph* g, F&& enqueue) {
  if (g->exec) {
    (void)hipGraphExecDestroy(g->exec);
    g->exec = nullptr;
  }
  if (!g->gs && hipStreamCreateWithFlags(&g->gs, hipStreamNonBlocking) != hipSuccess) return false;
  if (!g->ev_in && hipEventCreateWithFlags(&g->ev_in, hipEventDisableTiming) != hipSuccess) return false;
  if (!g->ev_out && hipEventCreateWithFlags(&g->ev_out, hipEventDisableTiming) != hipSuccess) return false;
  if (hipStreamBeginCapture(g->gs, hipStreamCaptureModeThreadLocal) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const int rc = enqueue(g->gs);
  hipGraph_t graph = nullptr;
  const hipError_t e = hipStreamEndCapture(g->gs, &graph);
  bool ok = rc == INS_OK && e == hipSuccess && graph != nullptr;
  if (ok) ok = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) == hipSuccess;
  if (graph) (void)hipGraphDestroy(graph);
  if (!ok) {
    (void)hipGetLastError();
    g->exec = nullptr;
  }
  return ok;
}

// nsteps steps of size dt with the final correction of every step but the last folded into the next step's first stage kernel
// (same arithmetic per cell; the uncorrected intermediate results never become visible).  Falls back to single steps elsewhere.
extern "C" int ins_rk_steps_f64(ins_rk_t* rk, double visc, double* u, double t, double dt, int nsteps, void* stream) {
  INS_REQUIRE(rk && u && nsteps >= 0, "bad argument");
  const ins_grid* G = rk->grid;
  hipStream_t s = as_stream(stream);
  // The in-kernel correction runs on the fused periodic loop of this box (boxes too narrow for the 64-wide stage kernel chain on the 62-wide one: it
  // stores the corrected start field too); a body force takes single steps.  rk->ext: this entry point never runs the extended loop, and its 2-D
  // condition has always turned an integrator with closure / temperature state away while the 3-D one never looked — both kept as they were.
  const bool chain = ins_rk_chainable(rk) && !rk->force && !(G->g.D == 2 && rk->ext);
  const int gkind = step_graph_kind(rk, chain && nsteps >= 2);
  if (gkind && nsteps >= 3) {
    StepGraph* sg = static_cast<StepGraph*>(rk->step_graph);
    if (!sg) rk->step_graph = sg = new StepGraph();
    int rc, done = 0;
    // first step: direct (kind 1: it leaves its result uncorrected for the chain)
    if ((rc = gkind == 1 ? chain_step(rk, visc, u, dt, s, 2) : ins_rk_step_f64(rk, visc, u, t, dt, nullptr, stream))) return rc;
    done = 1;
    const int last_direct = gkind == 1 ? 1 : 0;  // kind 1: the last step corrects (chain bit 1 only) and runs directly
    const int nreplay = nsteps - done - last_direct;
    const bool same = sg->exec && sg->u == u && sg->dt == dt && sg->visc == visc && sg->force == rk->force && sg->kind == gkind && sg->epoch == ins_opt_epoch();
    if (!same && !sg->broken) {
      const bool got = step_graph_capture(sg, [&](hipStream_t gs) {
        return gkind == 1 ? chain_step(rk, visc, u, dt, gs, 3) : ins_rk_step_f64(rk, visc, u, t, dt, nullptr, gs);
      });
      sg->u = u, sg->dt = dt, sg->visc = visc, sg->force = rk->force, sg->kind = gkind, sg->epoch = ins_opt_epoch();
      if (!got) sg->broken = true;
    }
    if (sg->exec && !sg->broken && nreplay > 0) {
      INS_HIP_TRY(hipEventRecord(sg->ev_in, s));
      INS_HIP_TRY(hipStreamWaitEvent(sg->gs, sg->ev_in, 0));
      for (int n = 0; n < nreplay; ++n) INS_HIP_TRY(hipGraphLaunch(sg->exec, sg->gs));
      INS_HIP_TRY(hipEventRecord(sg->ev_out, sg->gs));
      INS_HIP_TRY(hipStreamWaitEvent(s, sg->ev_out, 0));
      sg->replays += nreplay;
      done += nreplay;
    }
    for (int n = done; n < nsteps; ++n) {  // the last step of a chain, or everything when no graph exists
      if (gkind == 1)
        rc = chain_step(rk, visc, u, dt, s, 1 | (n < nsteps - 1 ? 2 : 0));
      else
        rc = ins_rk_step_f64(rk, visc, u, t + n * dt, dt, nullptr, stream);
      if (rc) return rc;
    }
    return INS_OK;
  }
  if (!chain || nsteps < 2) {
    for (int n = 0; n < nsteps; ++n) {
      int rc = ins_rk_step_f64(rk, visc, u, t + n * dt, dt, nullptr, stream);
      if (rc) return rc;
    }
    return INS_OK;
  }
  // the final gradient-subtract / ghost pass of every step but the last goes into the next step's first stage kernel
  for (int n = 0; n < nsteps; ++n) {
    int rc = chain_step(rk, visc, u, dt, s, (n > 0 ? 1 : 0) | (n < nsteps - 1 ? 2 : 0));
    if (rc) return rc;
  }
  return INS_OK;
}

// planes: nsets x 18 device pointers.  nsets == 1: the same boundary data for every ghost fill of the step; nsets == nstage + 1: set q holds the data at
// time tstart (q = 0) / tstart + c[q-1] Δt — the fill before stage i's momentum! reads set i (the OLD stage time, step_explicit_runge_kutta.jl:19), the fill
// before its projection and the final one read set i + 1 (:32, :48, :55).
static int rk_step_any(ins_rk_t* rk, double visc, double* u, double dt, const double* const* planes, int nsets, void* stream) {
  INS_REQUIRE(rk && u, "null argument");
  const ins_grid* G = rk->grid;
  hipStream_t s = as_stream(stream);
  if (!planes && ins_rk_fused3d(rk)) return rk_step_fused_periodic(rk, visc, u, dt, s);
  if (!planes && ins_rk_fused2d(rk)) return rk_step_fused_periodic_2d(rk, visc, u, dt, s);
  const long long nvec = G->ncell * G->g.D;
  DevBuf<const double*> dplanes;
  if (planes)
    if (int rc0 = dplanes.alloc_copy_host((size_t)nsets * 18, planes)) return rc0;
  auto pset = [&](int q) -> const double** { return dplanes ? dplanes + 18 * (nsets > 1 ? q : 0) : nullptr; };
  int rc;
  const int ns = rk->nstage;
  // Time-independent boundary data: K6 runs as K1's epilogue (no k_combine pass, no
  // snapshot copy: the caller's u is ustart for the whole step and the stage velocities ping-pong in two library buffers,
  // as on the periodic path).  Every non-interior volume of a stage buffer is (re)written by apply_bc_u! before it is read.
  const bool no_fuse_np = ins_opt(OPT_INS_DISABLE_FUSED_RK) != 0;
  const bool tiled = ins_fast3d_supported(G);  // else: the generic kernel with the same epilogue (2-D grids, tiny boxes)
  if (!no_fuse_np && !planes) {
    const size_t vbytes = (size_t)nvec * sizeof(double);
    if ((rc = ins_rk_ensure_ub(rk, vbytes, s, u))) return rc;
    // Masked grids with Periodic / Dirichlet sides and the direct solver: stages >= 2 read the previous stage's UNCORRECTED u* and its
    // pressure and apply `u = u* - ∇p` in registers on the degrees of freedom (CORR = 3 of the 62-wide stage kernel), so between two
    // stages the projection only solves for p: no gradient-subtract pass over u, no second ghost fill.  Same arithmetic per volume as
    // project! + apply_bc_u! (boundary data is time-independent on this entry point); INS_DISABLE_INKERNEL_CORR restores them.
    const bool incorr = tiled && ns > 1 && !ins_opt(OPT_INS_DISABLE_INKERNEL_CORR) && ins_corr3_supported(G) && ins_k_project_fdm_fused(rk->ps);
    // Stage-velocity basis (ins_rk_terms.h), as on the periodic path: with the in-kernel correction the uncorrected stage velocities V_m (boundary data
    // applied) stay in memory as the next stencil's input (on volumes that are no DOF every term holds the same boundary value and the weights sum to
    // one).  INS_RK_KEEP_K=1 restores the k-basis.
    const bool vbasis = incorr && !ins_opt(OPT_INS_RK_KEEP_K) && ins_rk_vbasis_possible(rk->A.data(), ns);
    double* cur = u;
    for (int i = 0; i < ns; ++i) {
      const bool corr_in = incorr && i > 0;
      if (!corr_in && (rc = ins_k_apply_bc_u(G, cur, 0, nullptr, s))) return rc;  // :19 (corr_in: `cur` got its boundary data at :48 already)
      double* out = (i == ns - 1 && ns > 1) ? u : (vbasis ? rk->ku[i] : rk->ub[i & 1]);
      // the V_m live in the ku arrays; the tiled kernels read V_{i-1} from memory like every other term (no self_in)
      RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, vbasis ? RK_V_BASIS : RK_K_BASIS, false, RK_FORCE_DIAG_FIRST);
      epi.ustart = (i == 0) ? nullptr : u;
      epi.ustar = out;
      rc = timed_stage(rk, s, [&] {  // :21, :35-38
        if (corr_in) return ins_k_momentum_rk_fused_corr3(G, visc, cur, rk->p, rk->ku[i], epi, s);
        if (tiled) return ins_k_momentum_rk_fused(G, visc, cur, rk->ku[i], epi, s);
        return ins_flux2d_supported(G) ? ins_k_flux2d(G, visc, cur, rk->ku[i], &epi, s) : ins_k_momentum_rk_fused_generic(G, visc, cur, rk->ku[i], epi, s);
      });
      if (rc) return rc;
      cur = out;
      if ((rc = ins_k_apply_bc_u(G, cur, 0, nullptr, s))) return rc;           // :48
      if (incorr && i < ns - 1)
        rc = ins_k_project_fdm_solve_only(G, rk->ps, cur, rk->p, s);            // :49 without its gradient-subtract
      else
        rc = ins_k_project(G, rk->ps, cur, rk->p, s);                           // :49
      if (rc) return rc;
    }
    if (ns == 1) INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], vbytes, hipMemcpyDeviceToDevice, s));
    return ins_k_apply_bc_u(G, u, 0, nullptr, s);                              // :55
  }
  // copyto!(ustart, u)                                                   step_explicit_runge_kutta.jl:14
  INS_HIP_TRY(hipMemcpyAsync(rk->ustart, u, nvec * sizeof(double), hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < ns; ++i) {
    if ((rc = ins_k_apply_bc_u(G, u, 0, pset(i), s))) return rc;             // :19
    // ku[i]'s ghost shell is zero from ins_rk_create and never written, so the fast path skips re-zeroing it
    rc = timed_stage(rk, s, [&] {
      return ins_fast3d_supported(G) ? ins_k_momentum_fast3d_opts(G, visc, u, rk->ku[i], false, s) : ins_k_momentum_generic(G, visc, u, rk->ku[i], s);  // :21
    });
    if (rc) return rc;
    Combine cb;                                                               // :35-38
    cb.n = ins_rk_sum_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, cb.coef, cb.k);
    const unsigned nblk = (unsigned)std::min<long long>((nvec / 2 + 255) / 256, 8192);
    hipLaunchKernelGGL(k_combine, dim3(nblk), dim3(256), 0, s, nvec, rk->ustart, u, cb);
    INS_LAUNCH_CHECK();
    if ((rc = ins_k_apply_bc_u(G, u, 0, pset(i + 1), s))) return rc;         // :48
    if ((rc = ins_k_project(G, rk->ps, u, rk->p, s))) return rc;              // :49
  }
  if ((rc = ins_k_apply_bc_u(G, u, 0, pset(ns), s))) return rc;              // :55
  if (planes) INS_HIP_TRY(hipStreamSynchronize(s));                           // dplanes is freed on return
  return INS_OK;
}

extern "C" int ins_rk_step_f64(ins_rk_t* rk, double visc, double* u, double t, double dt, const double* const* planes, void* stream) {
  (void)t;  // boundary data is time-independent on this entry point (see header)
  return rk_step_any(rk, visc, u, dt, planes, 1, stream);
}

// timestep! with time-dependent Dirichlet data (boundary_conditions.jl:351-357: bc.u(α, x..., t)): closures cannot cross the ABI, but the times at which
// the stage loop fills the ghost volumes are known before the step — tstart and tstart + c[i] Δt —, so the host evaluates its closures on the boundary
// planes for those nstage + 1 times and the whole stage loop runs here (the reference's kernel sequence: apply_bc_u!, momentum!, the combination,
// apply_bc_u!, project!).  planes_by_time: (nstage + 1) x 18 device pointers, entry (q·18 + (β·2 + side)·3 + α) as in ins_apply_bc_u_f64 (NULL: constant data).
extern "C" int ins_rk_step_bc_f64(ins_rk_t* rk, double visc, double* u, double t, double dt, const double* const* planes_by_time, void* stream) {
  INS_REQUIRE(rk && u && planes_by_time, "null argument");
  (void)t;
  return rk_step_any(rk, visc, u, dt, planes_by_time, rk->nstage + 1, stream);
}
