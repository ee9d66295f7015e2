// Ensemble stepping: B independent velocity fields of one 2-D periodic setup advanced by the chained loop of ins_rk_steps_f64 (ins_rk.hip,
// rk_step_fused_periodic_2d) with the member as one more launch dimension.  A 2-D RK44 step of a 64² .. 256² grid is a chain of dependent launches of a few
// microseconds each, with a few thousand cells of work behind every one of them: here every launch of that chain carries all B members, so the
// count per step is the single field's whatever B is.
//   * the stage kernel (ins_flux2d.hip, k_flux2d_members), the solve (ins_fft.hip k_xysolve2d / k_xfwd / k_xinv with MEMBERS, ins_zsolve.hip with MEANROWS)
//     and the last stage's gradient-subtract + ghost pass (ins_poisson.hip, k_grad_ghost with MEMBERS) are the single field's kernels instantiated with a
//     member index: per-cell and per-line arithmetic is the same text, row chunking, tile walks and FFT stage order depend on the grid only, so member b comes
//     out bitwise as ins_rk_steps_f64 leaves that field on its own (tests/test_gpu_ensemble.py);
//   * the handle owns every B-fold work array; of the solver it reads the route, the symbols and the twiddle tables and writes nothing.
#include "ins_debug.h"
#include "ins_internal.h"
#include "ins_rk_terms.h"

// struct ins_rk_ensemble: ins_internal.h (the observers of ins_rk_ensemble_observe.hip share it)

namespace {

// First-stage ghost fill of every member (apply_bc_u! on a periodic 2-D box, boundary_conditions.jl:276-288): direction be of all members in one launch,
// work-items along the full padded extent of the other direction (so the second direction also fills the corners), blockIdx.y = member, blockIdx.z = component.
__global__ __launch_bounds__(256) void k_bc_u_periodic2d_members(double* __restrict__ U, long long ustride, long long sc, int N0, int N1, int be) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= (be == 0 ? N1 : N0)) return;
  double* ua = U + (long long)blockIdx.y * ustride + (long long)blockIdx.z * sc;
  const long long base = be == 0 ? (long long)q * N0 : q, sb = be == 0 ? 1 : N0;
  const int last = (be == 0 ? N0 : N1) - 1;
  ua[base] = ua[base + (last - 1) * sb];
  ua[base + last * sb] = ua[base + sb];
}

// the arguments that need no handle: shared by the entries and the test hook
int check_args(long long ncell, int nbatch, long long ustride, int nsteps) {
  INS_REQUIRE(nbatch >= 1 && nbatch <= 65535, "an ensemble has 1 .. 65535 members");
  INS_REQUIRE(nsteps >= 0, "negative number of steps");
  INS_REQUIRE(ustride >= 2 * ncell, "member stride shorter than a vector field (2 ncell)");
  return INS_OK;
}

// the boxes of the chained 2-D loop, asked of the single-field predicates themselves
bool supported(const ins_grid* G, ins_poisson* ps, int nstage) {
  if (G->g.D != 2) return false;
  ins_rk probe;
  probe.grid = G;
  probe.ps = ps;
  probe.nstage = nstage;
  return ins_rk_fused2d(&probe) && ins_rk_inkernel2d(&probe);
}

int refuse(const char* why) {
  ins_set_error("ins_rk_ensemble: %s; the ensemble loop runs the boxes of the chained 2-D loop only (all-periodic, exactly uniform, power-of-two sides 16 .. 1024, "
                "spectral solver on its own passes, more than one stage): advance each member with ins_rk_steps_f64 (timesteps_ per member)", why);
  return INS_ERR_UNSUPPORTED;
}

// the same for the entries that run one link of the data-generation chain, not the stepper: the per-member route is the operator-level calls
int refuse_chain(const char* entry, const char* why) {
  ins_set_error("%s: %s; the member forms run the boxes of the chained 2-D loop only (all-periodic, exactly uniform, power-of-two sides 16 .. 1024, spectral "
                "solver on its own passes, more than one stage): run ins_momentum_f64, ins_apply_bc_u_f64 and ins_project_f64 on each member", entry, why);
  return INS_ERR_UNSUPPORTED;
}

// the same for the operator-level entries of the differentiable member step (ad.timestep_ensemble): the per-trajectory route is ad.timestep / create_loss_post
int refuse_ad(const char* entry, const char* why) {
  ins_set_error("%s: %s; the member operators run the boxes of the chained 2-D loop only (all-periodic, exactly uniform, power-of-two sides 16 .. 1024, spectral "
                "solver on its own passes, more than one stage): differentiate each trajectory on its own (ad.timestep, create_loss_post: ins_momentum_f64, "
                "ins_project_f64 and their pullbacks ins_momentum_pullback_f64, ins_apply_bc_u_pullback_f64, ins_project_pullback_f64 on each member)", entry, why);
  return INS_ERR_UNSUPPORTED;
}

// the same for the observers (ensemble_stats, observespectrum_ensemble): the per-member route is the single-field diagnostics
int refuse_observe(const char* entry, const char* why) {
  ins_set_error("%s: %s; the member observers run the boxes of the chained 2-D loop only (all-periodic, exactly uniform, power-of-two sides 16 .. 1024, spectral "
                "solver on its own passes, more than one stage): observe each member on its own (ins_total_kinetic_energy_f64, ins_max_abs_divergence_f64, "
                "ins_cfl_timestep_f64 and ins_spectrum_f64 on each member)", entry, why);
  return INS_ERR_UNSUPPORTED;
}

// Does a member of `out` (nb members of len elements, so apart) share an element with a member of `in` (si apart)?  The kernels read neighbours of what other
// work-items write, so an output may not overlap an input anywhere, not only at the base pointers.  Both strides are >= len (check_args), so member i of `out`,
// which starts a elements behind `in`, can only meet members floor(a / si) and floor(a / si) + 1 of `in`.
bool members_overlap(const double* out, long long so, const double* in, long long si, int nb, long long len) {
  const long long d = (long long)(((intptr_t)out - (intptr_t)in) / (intptr_t)sizeof(double));
  for (int i = 0; i < nb; ++i) {
    const long long a = d + (long long)i * so;
    const long long j0 = a >= 0 ? a / si : -((-a + si - 1) / si);
    for (long long j = j0; j <= j0 + 1; ++j)
      if (j >= 0 && j < nb && a < j * si + len && j * si < a + len) return true;
  }
  return false;
}

// the checks every operator-level entry makes of one ensemble field and of the handle's box
int check_entry(const ins_rk_ensemble* e, const char* entry, std::initializer_list<long long> strides) {
  for (const long long st : strides) {
    const int rc = check_args(e->grid->ncell, e->nb, st, 0);
    if (rc) return rc;
  }
  if (!supported(e->grid, e->ps, e->nstage)) return refuse_ad(entry, "an option has switched the chained 2-D loop off since the handle was created");
  return INS_OK;
}

// Transpose of k_bc_u_periodic2d_members in direction be: the copies x[0] = x[last-1]; x[last] = x[1] become, in reverse order, x̄[1] += x̄[last], x̄[last] = 0,
// then x̄[last-1] += x̄[0], x̄[0] = 0 — the arithmetic of k_bc_u_pullback<2, double> on a periodic line.  Same launch shape as the forward.
__global__ __launch_bounds__(256) void k_bc_u_periodic2d_members_pullback(double* __restrict__ G, long long gstride, long long sc, int N0, int N1, int be) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= (be == 0 ? N1 : N0)) return;
  double* ga = G + (long long)blockIdx.y * gstride + (long long)blockIdx.z * sc;
  const long long base = be == 0 ? (long long)q * N0 : q, sb = be == 0 ? 1 : N0;
  const int last = (be == 0 ? N0 : N1) - 1;
  const double r = ga[base + last * sb];
  ga[base + last * sb] = 0.0;
  ga[base + sb] += r;
  const double l = ga[base];
  ga[base] = 0.0;
  ga[base + (last - 1) * sb] += l;
}

// the ghost fill's transpose for all members: direction 1, then direction 0 (the reverse of fill_ghosts), two launches whatever nb is
int fold_ghosts(const ins_rk_ensemble* e, double* G, long long gstride, hipStream_t s) {
  const GridDev& g = e->grid->g;
  for (int be = 1; be >= 0; --be) {
    const dim3 grid(cdiv(g.N[be == 0 ? 1 : 0], 256), (unsigned)e->nb, 2);
    hipLaunchKernelGGL(k_bc_u_periodic2d_members_pullback, grid, dim3(256), 0, s, G, gstride, g.sc, g.N[0], g.N[1], be);
    INS_LAUNCH_CHECK();
  }
  return INS_OK;
}

int fill_ghosts(const ins_rk_ensemble* e, double* U, long long ustride, hipStream_t s) {
  const GridDev& g = e->grid->g;
  for (int be = 0; be < 2; ++be) {
    const dim3 grid(cdiv(g.N[be == 0 ? 1 : 0], 256), (unsigned)e->nb, 2);
    hipLaunchKernelGGL(k_bc_u_periodic2d_members, grid, dim3(256), 0, s, U, ustride, g.sc, g.N[0], g.N[1], be);
    INS_LAUNCH_CHECK();
  }
  return INS_OK;
}

// One step of all members: rk_step_fused_periodic_2d (ins_rk.hip) launch for launch.  chain as there: bit 1 = U holds the previous step's uncorrected
// result and pI its pressure; bit 2 = leave this step's result uncorrected.
int step(ins_rk_ensemble* e, double visc, double* U, long long ustride, double dt, hipStream_t s, int chain) {
  const ins_grid* G = e->grid;
  const int ns = e->nstage;
  const long long np = (long long)e->ps->np[0] * e->ps->np[1];
  const bool raw_in = chain & 1, raw_out = chain & 2;
  int rc;
  if (!raw_in && (rc = fill_ghosts(e, U, ustride, s))) return rc;
  const double* in = U;
  long long in_stride = ustride;
  for (int i = 0; i < ns; ++i) {
    const bool last = i == ns - 1;
    double* out = last ? U : e->ub[i & 1];
    const long long out_stride = last ? ustride : e->ms;
    RkEpi epi = ins_rk_stage_terms(e->A.data(), ns, i, dt, e->ku, (const double*)nullptr, RK_K_BASIS, false, RK_FORCE_INDEX_ORDER);
    epi.ustart = (i == 0) ? nullptr : (raw_in ? e->ustart : U);
    epi.ustar = out;
    if (i == 0 && raw_in) epi.ustart_out = e->ustart;
    const bool corr = i > 0 || raw_in;
    const RkMemberStrides st = {in_stride, corr ? np : 0, e->ms, raw_in ? e->ms : ustride, e->ms, out_stride, e->ms};
    if ((rc = ins_k_flux2d_members(G, visc, in, e->ku[i], epi, s, corr ? e->pI : nullptr, e->nb, st))) return rc;
    if ((rc = ins_k_solve_members_2d(G, e->ps, out, out_stride, e->nb, e->pI, e->phat, e->zrows, s))) return rc;
    if (last && !raw_out && (rc = ins_k_grad_ghost_members_2d(G, e->ps, out, out_stride, e->nb, e->pI, s))) return rc;
    in = out;
    in_stride = out_stride;
  }
  return INS_OK;
}

}  // namespace

int ins_rk_ensemble_check_observer(const ins_rk_ensemble* e, const char* entry, long long ustride) {
  const int rc = check_args(e->grid->ncell, e->nb, ustride, 0);
  if (rc) return rc;
  if (!supported(e->grid, e->ps, e->nstage)) return refuse_observe(entry, "an option has switched the chained 2-D loop off since the handle was created");
  return INS_OK;
}

extern "C" int ins_dbg_rk_ensemble_args(int64_t ncell, int32_t nbatch, int64_t ustride, int32_t nsteps) { return check_args(ncell, nbatch, ustride, nsteps); }

extern "C" int ins_rk_ensemble_create(const ins_grid_t* G, ins_poisson_t* ps, int nstage, const double* A, const double* c, int nbatch, ins_rk_ensemble_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  int rc = check_args(G->ncell, nbatch, 2 * G->ncell, 0);
  if (rc) return rc;
  INS_REQUIRE(nstage >= 1 && nstage <= INS_MAX_STAGES, "unsupported number of stages");
  for (int i = 0; i < nstage; ++i)
    for (int j = i + 1; j < nstage; ++j) INS_REQUIRE(A[i * nstage + j] == 0.0, "shifted tableau must be lower triangular (explicit method)");
  if (G->g.D != 2) return refuse("a 3-D grid");
  if (nstage < 2) return refuse("a one-stage method");
  if (!supported(G, ps, nstage)) return refuse("this grid / solver does not run the chained 2-D loop");
  ins_rk_ensemble* e = new ins_rk_ensemble();
  e->grid = G;
  e->ps = ps;
  e->nstage = nstage;
  e->nb = nbatch;
  e->A.assign(A, A + nstage * nstage);
  e->c.assign(c, c + nstage);
  e->ms = 2 * G->ncell;
  const size_t nvec = (size_t)e->ms * nbatch;
  const size_t npre = (size_t)ps->np[0] * ps->np[1] * nbatch;
  const size_t nhat = (size_t)ps->kxs * ps->np[1] * nbatch * 2;
  // every array zeroed once: ghost rings and padding columns that no kernel writes are read by none either, but hold defined values
  (rc = e->ustart.alloc_zero(nvec)) || (rc = e->ub[0].alloc_zero(nvec)) || (rc = e->ub[1].alloc_zero(nvec)) || (rc = e->pI.alloc_zero(npre)) ||
      (rc = e->zrows.alloc_zero(nbatch));
  if (rc == INS_OK && ps->route == ROUTE_OWN2D) rc = e->phat.alloc_zero(nhat);
  e->ku.resize(nstage);
  for (int i = 0; rc == INS_OK && i < nstage; ++i) rc = e->ku[i].alloc_zero(nvec);
  if (rc != INS_OK) {
    ins_rk_ensemble_destroy(e);
    return rc;
  }
  *out = e;
  return INS_OK;
}

extern "C" int ins_rk_ensemble_destroy(ins_rk_ensemble_t* e) {
  if (!e) return INS_OK;
  delete e;
  return INS_OK;
}

// nsteps steps of every member: the loop of ins_rk_steps_f64 — chained (the final gradient-subtract / ghost pass of every step but the last goes into the next
// step's first stage kernel) where that entry chains a single field, whole steps where it does not (one step, INS_DISABLE_STEP_CHAIN).
extern "C" int ins_rk_ensemble_steps_f64(ins_rk_ensemble_t* e, double visc, double* U, int64_t ustride, double t, double dt, int nsteps, void* stream) {
  (void)t;  // no boundary data, no force: nothing depends on time
  INS_REQUIRE(e && U, "null argument");
  int rc = check_args(e->grid->ncell, e->nb, ustride, nsteps);
  if (rc) return rc;
  // the switches that shape the single-field loop are read per call there; a handle whose box they have since turned away is refused, not run another way
  if (!supported(e->grid, e->ps, e->nstage)) return refuse("an option has switched the chained 2-D loop off since the handle was created");
  hipStream_t s = as_stream(stream);
  const bool chain = !ins_opt(OPT_INS_DISABLE_STEP_CHAIN) && nsteps >= 2;
  for (int n = 0; n < nsteps; ++n)
    if ((rc = step(e, visc, U, ustride, dt, s, chain ? ((n > 0 ? 1 : 0) | (n < nsteps - 1 ? 2 : 0)) : 0))) return rc;
  return INS_OK;
}

// The projected right-hand side of every member, F[b] = apply_bc_u!(project!(apply_bc_u!(momentum!(U[b]); dudt))): what filtersaver and lesdatagen form per saved
// state (data_generation.jl:37-60, 62-120), on the member forms the step drives and on the handle's own pI / phat.  Launches: the force form of the stage
// kernel, the solve (one pass or three) and the gradient-subtract + ghost pass, whatever nb is.  On a periodic box the solve reads the interior of F through
// its periodic images and the last pass writes every ghost volume of F, so the ghost fill between momentum! and project! of the per-member chain has no reader
// and is not launched.  U is read only (ghosts valid); F's padding between members is not touched.
extern "C" int ins_rk_ensemble_rhs_f64(ins_rk_ensemble_t* e, double visc, const double* U, int64_t ustride, double* F, int64_t fstride, void* stream) {
  INS_REQUIRE(e && U && F, "null argument");
  INS_REQUIRE(U != F, "the right-hand side cannot be formed in place");
  int rc = check_args(e->grid->ncell, e->nb, ustride, 0);
  if (rc || (rc = check_args(e->grid->ncell, e->nb, fstride, 0))) return rc;
  if (!supported(e->grid, e->ps, e->nstage)) return refuse_chain("ins_rk_ensemble_rhs_f64", "an option has switched the chained 2-D loop off since the handle was created");
  hipStream_t s = as_stream(stream);
  if ((rc = ins_k_flux2d_members_force(e->grid, visc, U, ustride, F, fstride, e->nb, s))) return rc;
  if ((rc = ins_k_solve_members_2d(e->grid, e->ps, F, fstride, e->nb, e->pI, e->phat, e->zrows, s))) return rc;
  return ins_k_grad_ghost_members_2d(e->grid, e->ps, F, fstride, e->nb, e->pI, s);
}

// apply_bc_u! of every member on the periodic box (boundary_conditions.jl:276-288): the first-stage ghost fill of the step as an entry of its own, for fields
// that reach the ensemble from elsewhere with their interior only (filtered fields: the filters write Iu[α]).  Two launches whatever nb is.
extern "C" int ins_rk_ensemble_apply_bc_u_f64(ins_rk_ensemble_t* e, double* U, int64_t ustride, void* stream) {
  INS_REQUIRE(e && U, "null argument");
  int rc = check_args(e->grid->ncell, e->nb, ustride, 0);
  if (rc) return rc;
  if (!supported(e->grid, e->ps, e->nstage)) return refuse_chain("ins_rk_ensemble_apply_bc_u_f64", "an option has switched the chained 2-D loop off since the handle was created");
  return fill_ghosts(e, U, ustride, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// The operators of one differentiable step of all members (ad.timestep_ensemble) and their pullbacks.  Each entry costs the launches of one field whatever nb is.
// ------------------------------------------------------------------------------------------------
// F[b] = momentum!(U[b]) on the interior of every member (the force form of the stage kernel): U has valid ghosts and is read only, the ghost ring of F is untouched.
extern "C" int ins_rk_ensemble_momentum_f64(ins_rk_ensemble_t* e, double visc, const double* U, int64_t ustride, double* F, int64_t fstride, void* stream) {
  INS_REQUIRE(e && U && F, "null argument");
  const int rc = check_entry(e, "ins_rk_ensemble_momentum_f64", {ustride, fstride});
  if (rc) return rc;
  INS_REQUIRE(!members_overlap(F, fstride, U, ustride, e->nb, 2 * e->grid->ncell), "momentum of the members cannot be formed in place: a member of F overlaps a member of U");
  return ins_k_flux2d_members_force(e->grid, visc, U, ustride, F, fstride, e->nb, as_stream(stream));
}

// U[b] <- apply_bc_u(project(apply_bc_u(U[b]))) in place: the member solve, which reads the interior of U through its periodic images, then the
// gradient-subtract + ghost pass, on the handle's pI / phat (the last two calls of ins_rk_ensemble_rhs_f64).
extern "C" int ins_rk_ensemble_project_f64(ins_rk_ensemble_t* e, double* U, int64_t ustride, void* stream) {
  INS_REQUIRE(e && U, "null argument");
  int rc = check_entry(e, "ins_rk_ensemble_project_f64", {ustride});
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  if ((rc = ins_k_solve_members_2d(e->grid, e->ps, U, ustride, e->nb, e->pI, e->phat, e->zrows, s))) return rc;
  return ins_k_grad_ghost_members_2d(e->grid, e->ps, U, ustride, e->nb, e->pI, s);
}

// The transpose of ins_rk_ensemble_apply_bc_u_f64 on the padded arrays, in place: ghost cotangents are added to the interior volumes they were copied from and
// zeroed, direction 1 before direction 0.
extern "C" int ins_rk_ensemble_apply_bc_u_pullback_f64(ins_rk_ensemble_t* e, double* G, int64_t gstride, void* stream) {
  INS_REQUIRE(e && G, "null argument");
  const int rc = check_entry(e, "ins_rk_ensemble_apply_bc_u_pullback_f64", {gstride});
  if (rc) return rc;
  return fold_ghosts(e, G, gstride, as_stream(stream));
}

// Ubar[b] (+)= J_F(U[b])ᵀ Phibar[b] over the whole padded array of every member, the contract of ins_momentum_pullback_f64, in one launch.
extern "C" int ins_rk_ensemble_momentum_pullback_f64(ins_rk_ensemble_t* e, double visc, const double* U, int64_t ustride, const double* Phibar, int64_t pstride,
                                                     double* Ubar, int64_t bstride, int accumulate, void* stream) {
  INS_REQUIRE(e && U && Phibar && Ubar, "null argument");
  const int rc = check_entry(e, "ins_rk_ensemble_momentum_pullback_f64", {ustride, pstride, bstride});
  if (rc) return rc;
  const long long len = 2 * e->grid->ncell;
  INS_REQUIRE(!members_overlap(Ubar, bstride, U, ustride, e->nb, len) && !members_overlap(Ubar, bstride, Phibar, pstride, e->nb, len),
              "momentum pullback cannot run in place: a member of Ubar overlaps a member of U or Phibar");
  return ins_k_momentum_pullback_members_2d(e->grid, visc, U, ustride, Phibar, pstride, Ubar, bstride, accumulate != 0, e->nb, as_stream(stream));
}

// The exact transpose of ins_rk_ensemble_project_f64 on the padded arrays, in place.  The forward is E·P·R: R restricts to the interior (the solve forms the
// divergence through the periodic wrap and reads no ghost volume: k_xfwd / k_xysolve2d with XSRC_DIV_2D), P = I − G L⁻¹ Ω D is the periodic projection, which
// is symmetric on an exactly uniform grid (Ω constant, G = −Dᵀ), and E is the periodic extension written by the last pass.  So the transpose is Rᵀ·P·Eᵀ: fold
// the ghost cotangents into the interior, the SAME member solve and gradient-subtract on the folded cotangent, every ghost volume zero.
// Launches: the forward's plus the two of the fold.
extern "C" int ins_rk_ensemble_project_pullback_f64(ins_rk_ensemble_t* e, double* G, int64_t gstride, void* stream) {
  INS_REQUIRE(e && G, "null argument");
  int rc = check_entry(e, "ins_rk_ensemble_project_pullback_f64", {gstride});
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  if ((rc = fold_ghosts(e, G, gstride, s))) return rc;
  if ((rc = ins_k_solve_members_2d(e->grid, e->ps, G, gstride, e->nb, e->pI, e->phat, e->zrows, s))) return rc;
  return ins_k_grad_zero_ghost_members_2d(e->grid, e->ps, G, gstride, e->nb, e->pI, s);
}
