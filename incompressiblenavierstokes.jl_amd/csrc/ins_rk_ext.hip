// Native stage loop that carries the temperature equation and the Smagorinsky closure:
// timestep!(method::ExplicitRungeKuttaMethod, stepper, Δt) with `temp` and / or `closure_model` set
// (step_explicit_runge_kutta.jl:4-59), boundary data time-independent.  Per stage i
//   apply_bc_u!, apply_bc_temp!                                                       :19-20
//   ku[i] = momentum(u, temp) = convection-diffusion + body force + gravity(temp)      :21   (operators.jl:967-976)
//   ktemp[i] = convection_diffusion_temp(u, temp) + dissipation(u)                     :23-27
//   ku[i] += closure(u, θ) = divoftensor(apply_bc_p(smagtensor(u, θ)))                 :31-34 (operators.jl:1294-1305)
//   u = ustart + Σ_j Δt A[i,j] ku[j],  temp = tempstart + Σ_j Δt A[i,j] ktemp[j]        :35-44
//   apply_bc_u!, project!                                                              :48-49
// and apply_bc_u!, apply_bc_temp! at the end (:55-56).  The host mirror drove exactly this from Python with one C-ABI call per
// operator; here the loop is one call, and on periodic uniform 3-D boxes with the spectral solver it runs on the fused kernels of the
// plain path: the closure term and gravity go into ONE vector field E_i that the stage kernel adds to its force in registers
// (RkEpi::extra: k_i = F_i + E_i is what is combined and stored — no axpy pass, no combine pass, no snapshot copy), the divergence is
// formed inside the solver's x pass and the gradient-subtract fills the ghost volumes (ins_k_project_periodic_fused).  The in-register
// pressure correction of the plain path does not apply: closure and temperature kernels need the corrected stage velocity in memory.
#include <cstring>
#include <vector>

#include "ins_debug.h"
#include "ins_internal.h"
#include "ins_rk_terms.h"

struct ins_rk_ext {
  int closure = 0;  // 0 none, 1 Smagorinsky
  double theta = 0.0;
  bool temp_on = false;
  ins_temperature_desc_t td;
  DevBuf<double> sigma;      // D(D+1)/2 scalar fields
  DevBuf<double> E;          // closure term + gravity (vector field)
  DevBuf<double> diff;       // scratch of dissipation! (vector field)
  DevBuf<double> tempstart;  // scalar
  DevBuf<double> w;          // u · diffusion(u) (vector field, written by the stage kernel; fused path)
  DevBuf<double> tb[2];      // stage temperatures (fused path)
  std::vector<DevBuf<double>> ktemp;  // nstage scalars
};

void ins_rk_ext_free(ins_rk_ext* e) { delete e; }

static ins_rk_ext* ext_of(ins_rk* rk) {
  if (!rk->ext) rk->ext = new ins_rk_ext();
  return rk->ext;
}

extern "C" int ins_rk_set_closure(ins_rk_t* rk, int32_t kind, double theta) {
  INS_REQUIRE(rk, "null argument");
  INS_REQUIRE(kind == 0 || kind == 1, "closure kind: 0 (none) or 1 (Smagorinsky)");
  ins_rk_ext* e = ext_of(rk);
  e->closure = kind;
  e->theta = theta;
  return INS_OK;
}

extern "C" int ins_rk_set_temperature(ins_rk_t* rk, const ins_temperature_desc_t* desc) {
  INS_REQUIRE(rk, "null argument");
  ins_rk_ext* e = ext_of(rk);
  e->temp_on = desc != nullptr;
  if (desc) {
    INS_REQUIRE(desc->gdir >= 0 && desc->gdir < rk->grid->g.D, "gdir out of range");
    e->td = *desc;
  }
  return INS_OK;
}

static long long g_fused_steps = 0, g_tiled_steps = 0;
extern "C" long long ins_dbg_ext_tiled_steps(void) { return g_tiled_steps; }
// test hook: how many steps took the fused path (periodic uniform 3-D boxes, spectral solver)
extern "C" long long ins_dbg_ext_fused_steps(void) { return g_fused_steps; }

// first use of a buffer: allocated and zeroed on the stream
static int zalloc(DevBuf<double>* b, size_t bytes, hipStream_t s) { return *b ? INS_OK : b->alloc_zero_async(bytes / sizeof(double), s); }

extern "C" int ins_rk_step_ext_f64(ins_rk_t* rk, double visc, double* u, double* temp, double t, double dt, void* stream) {
  INS_REQUIRE(rk && u, "null argument");
  ins_rk_ext* e = rk->ext;
  const bool closure = e && e->closure == 1, with_temp = e && e->temp_on;
  INS_REQUIRE(with_temp == (temp != nullptr), "a temperature field needs ins_rk_set_temperature and vice versa");
  if (!closure && !with_temp) return ins_rk_step_f64(rk, visc, u, t, dt, nullptr, stream);
  const ins_grid* G = rk->grid;
  const GridDev& g = G->g;
  hipStream_t s = as_stream(stream);
  const int ns = rk->nstage, D = g.D;
  const size_t sbytes = (size_t)G->ncell * sizeof(double), vbytes = sbytes * D;
  int rc;
  // the stress scratch (D(D+1)/2 scalar fields: 6.5 GB at 512^3) exists only where the three-kernel closure runs (the one-kernel form keeps σ in registers)
  auto need_sigma = [&]() { return zalloc(&e->sigma, sbytes * (D * (D + 1) / 2), s); };
  if (closure && (rc = zalloc(&e->E, vbytes, s))) return rc;
  if (with_temp) {
    if ((rc = zalloc(&e->tempstart, sbytes, s))) return rc;
    if (e->td.dodissipation && (rc = zalloc(&e->diff, vbytes, s))) return rc;
    if ((int)e->ktemp.size() < ns) e->ktemp.resize(ns);
    for (int i = 0; i < ns; ++i)
      if ((rc = zalloc(&e->ktemp[i], sbytes, s))) return rc;
    INS_HIP_TRY(hipMemcpyAsync(e->tempstart, temp, sbytes, hipMemcpyDeviceToDevice, s));  // state_copyto!(xstart, x)   :14
  }
  const ins_temperature_desc_t& td = e->td;
  auto bc_temp = [&]() { return with_temp ? ins_apply_bc_temp_f64(G, td.bc, td.val, nullptr, temp, stream) : INS_OK; };
  auto temp_rhs = [&](const double* v, int i) -> int {
    if (!with_temp) return INS_OK;
    int r;
    INS_HIP_TRY(hipMemsetAsync(e->ktemp[i], 0, sbytes, s));
    if ((r = ins_convection_diffusion_temp_f64(G, td.a4, v, temp, e->ktemp[i], stream))) return r;
    if (td.dodissipation && (r = ins_dissipation_f64(G, visc, td.diss_coef, v, e->diff, e->ktemp[i], stream))) return r;
    return INS_OK;
  };
  auto temp_combine = [&](int i) -> int {
    if (!with_temp) return INS_OK;
    double coefs[INS_MAX_STAGES];
    const double* ks[INS_MAX_STAGES];
    int n = 0;
    for (int j = 0; j <= i; ++j) {
      coefs[n] = dt * rk->A[i * ns + j];
      ks[n] = e->ktemp[j];
      ++n;
    }
    return ins_combine_scalar_f64(G, e->tempstart, temp, n, coefs, ks, stream);
  };

  // the plain fused periodic loop's boxes, where the 64-wide stage kernel runs (it carries the closure field, gravity and the temperature stage)
  const bool fused = ins_rk_fused3d(rk) && !ins_opt(OPT_INS_DISABLE_EXT_FUSED) && ins_flux64_supported(G);

  if (fused) {
    // Periodic uniform 3-D box, spectral solver.  Per stage: [closure kernels ->] stage kernel (convection-diffusion + closure field + gravity
    // from temp in registers, RK combination, and w = u · diffusion(u) as a by-product) -> one temperature kernel (its right-hand side and its
    // RK combination) -> the five solver passes -> gradient-subtract with ghost fill -> temperature ghost fill.
    ++g_fused_steps;
    if ((rc = ins_rk_ensure_ub(rk, vbytes, s, nullptr))) return rc;
    if (with_temp) {
      for (int b = 0; b < 2; ++b)
        if ((rc = zalloc(&e->tb[b], sbytes, s))) return rc;
      if (td.dodissipation && (rc = zalloc(&e->w, vbytes, s))) return rc;
    }
    if ((rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;
    if ((rc = bc_temp())) return rc;
    // Stage-velocity basis (ins_rk_terms.h): the projection writes the corrected field to another array, so the uncorrected stage
    // velocities V_m stay in memory (in the ku arrays) and no k_j is stored or read; INS_RK_KEEP_K=1 restores the k-basis.
    const bool vbasis = ns > 1 && !ins_opt(OPT_INS_RK_KEEP_K) && ins_rk_vbasis_possible(rk->A.data(), ns);
    // Every consumer of the stage velocity can correct it on the fly (the stage kernel as on the plain path, the split temperature kernel for
    // its two face velocities, the stress-tensor kernel through periodic images), so the gradient-subtract pass runs for the last stage only —
    // except when the temperature stage rides inside the stage kernel (it has no correcting variant).
    // The temperature stage itself rides inside the stage kernel (TempEpi: T as a fourth register component, the lower-face dissipation terms
    // from the halo column / halo row / previous plane); INS_EXT_TEMP_SPLIT=1 keeps it as a kernel of its own (then without a closure the
    // gradient-subtract passes between the stages can go, see above).
    const bool tin_kernel = with_temp && !ins_opt(OPT_INS_EXT_TEMP_SPLIT);
    // (with a closure and no temperature equation the stress-tensor kernel corrects on the fly as well: ins_k_smagtensor_corr)
    // The closure force as one kernel (ins_smagforce.hip: the stress never leaves the registers; it corrects on the fly like the stress-tensor
    // kernel, from the uncorrected stage velocity and its pressure)
    const bool smag1 = closure && ins_smagforce_supported(G);
    const bool incorr = vbasis && !tin_kernel && !ins_opt(OPT_INS_DISABLE_INKERNEL_CORR) && g.N[0] >= 34 && g.N[1] >= 8 && g.N[2] >= 8;
    const double* in = u;
    const double* tin = temp;
    for (int i = 0; i < ns; ++i) {
      const bool last = i == ns - 1 && ns > 1;
      double* out = last ? u : (vbasis ? rk->ku[i] : rk->ub[i & 1]);      // what the stage kernel writes (uncorrected)
      double* corrected = (last || incorr) ? out : rk->ub[i & 1];          // what the projection leaves (K4 route: with ghost volumes)
      double* tout = with_temp ? (last ? temp : e->tb[i & 1]) : nullptr;
      const bool corr_in = incorr && i > 0;  // `in` is the uncorrected V_{i-1}, ps->pI its pressure
      if (smag1) {
        if ((rc = ins_k_smagforce(G, e->theta, in, corr_in ? rk->ps->pI.get() : nullptr, e->E, s))) return rc;
      } else if (closure) {
        if ((rc = need_sigma())) return rc;
        rc = corr_in ? ins_k_smagtensor_corr(G, e->theta, in, rk->ps->pI, e->sigma, s) : ins_smagtensor_f64(G, e->theta, in, e->sigma, stream);
        if (rc) return rc;
        if ((rc = ins_k_apply_bc_p_fields(G, e->sigma, D * (D + 1) / 2, s))) return rc;  // apply_bc_p!(σ, 0, setup)   operators.jl:1302
        if ((rc = ins_divoftensor_f64(G, e->sigma, e->E, stream))) return rc;
      }
      // the V_m live in the ku arrays; V_{i-1} comes from registers where it is this stage's uncorrected stencil input (corr_in), else the stencil reads
      // the projection's corrected copy and V_{i-1} is a term like the others.  The steady force is not part of what is stored.
      RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, vbasis ? RK_V_BASIS : RK_K_BASIS, corr_in, RK_FORCE_DIAG_FIRST);
      epi.ustart = (i == 0) ? nullptr : u;
      epi.ustar = out;
      epi.extra = closure ? e->E : nullptr;
      TempEpi te;
      if (with_temp) {
        epi.gtemp = tin;
        epi.ga2 = td.a2;
        epi.gdir = td.gdir;
        if (tin_kernel) {
          memset(&te, 0, sizeof(te));
          te.temp = tin;
          te.tempstart = e->tempstart;
          te.temp_out = tout;
          te.ktemp_out = ins_rk_needed_later(rk->A.data(), ns, i) ? e->ktemp[i].get() : nullptr;
          for (int j = 0; j < i; ++j) {
            const double c = dt * rk->A[i * ns + j];
            if (c == 0.0) continue;
            te.coef[te.n] = c;
            te.k[te.n] = e->ktemp[j];
            ++te.n;
          }
          te.c_self = dt * rk->A[i * ns + i];
          te.a4 = td.a4;
          te.dcoef = td.dodissipation ? td.diss_coef : 0.0;
          epi.tstage = &te;
        } else {
          epi.wout = td.dodissipation ? e->w : nullptr;
        }
      }
      rc = corr_in ? ins_k_momentum_rk_fused_corr(G, visc, in, rk->ps->pI, rk->ku[i], epi, s) : ins_k_momentum_rk_fused(G, visc, in, rk->ku[i], epi, s);
      if (rc) return rc;
      if (with_temp && !tin_kernel) {
        double coefs[INS_MAX_STAGES];
        const double* ks[INS_MAX_STAGES];
        int n = 0;
        for (int j = 0; j < i; ++j) {
          coefs[n] = dt * rk->A[i * ns + j];
          ks[n] = e->ktemp[j];
          ++n;
        }
        const bool later = ins_rk_needed_later(rk->A.data(), ns, i);
        if ((rc = ins_k_temp_stage(G, td.a4, td.diss_coef, in, tin, td.dodissipation ? e->w : nullptr, e->tempstart, n, coefs, ks, dt * rk->A[i * ns + i],
                                   later ? e->ktemp[i].get() : nullptr, tout, s, corr_in ? rk->ps->pI.get() : nullptr)))
          return rc;
      }
      if (incorr && i < ns - 1)
        rc = ins_k_project_periodic_solve_only(G, rk->ps, out, s);
      else
        rc = ins_k_project_periodic_fused(G, rk->ps, out, rk->p, i == ns - 1, s, corrected == out ? nullptr : corrected);
      if (rc) return rc;
      if (with_temp && (rc = ins_apply_bc_temp_f64(G, td.bc, td.val, nullptr, tout, stream))) return rc;
      in = corrected;
      tin = tout;
    }
    if (ns == 1) {
      INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], vbytes, hipMemcpyDeviceToDevice, s));
      if (with_temp) INS_HIP_TRY(hipMemcpyAsync(temp, e->tb[0], sbytes, hipMemcpyDeviceToDevice, s));
    }
    return INS_OK;
  }

  // 3-D grids the tiled stage kernels take (walls, stretched grids, any solver): K1 + K6 + the extra force field in one stage kernel (the caller's u
  // is ustart for the whole step, stage velocities ping-pong in two library buffers: no snapshot copy, no combination pass, no axpy), one
  // temperature kernel per stage (right-hand side from (u, temp, diffusion(u)) + its RK combination), full projection after every stage.
  if (!ins_opt(OPT_INS_DISABLE_FUSED_RK) && !ins_opt(OPT_INS_DISABLE_EXT_FUSED) && D == 3 && ins_fast3d_supported(G)) {
    if ((rc = ins_rk_ensure_ub(rk, vbytes, s, u))) return rc;
    if (with_temp) {
      for (int b = 0; b < 2; ++b)
        if (!e->tb[b]) {
          if ((rc = e->tb[b].alloc_copy_device(sbytes / sizeof(double), temp, s))) return rc;
        }
    }
    // The 64-wide masked stage kernel also leaves w = u·diffusion(u) (the dissipation term of the temperature equation) from
    // the diffusive parts of the fluxes it has in registers: no diffusion pass of its own.
    const bool w_from_stage = with_temp && td.dodissipation && ins_flux64m_supported(G);
    if (w_from_stage && (rc = zalloc(&e->w, vbytes, s))) return rc;  // ghost volumes stay zero (the reference's fill!(diff, 0))
    ++g_tiled_steps;
    double* cur = u;
    double* tin = temp;
    for (int i = 0; i < ns; ++i) {
      const bool last = i == ns - 1 && ns > 1;
      double* out = last ? u : rk->ub[i & 1];
      double* tout = with_temp ? (last ? temp : e->tb[i & 1]) : nullptr;
      if ((rc = ins_k_apply_bc_u(G, cur, 0, nullptr, s))) return rc;                                         // :19
      if (with_temp && (rc = ins_apply_bc_temp_f64(G, td.bc, td.val, nullptr, tin, stream))) return rc;      // :20
      if (closure && ins_smagforce_supported(G)) {  // one kernel, also with walls and on stretched grids (ins_smagforce.hip, GEN)
        if ((rc = ins_k_smagforce(G, e->theta, cur, nullptr, e->E, s))) return rc;
      } else if (closure) {
        if ((rc = need_sigma())) return rc;
        if ((rc = ins_smagtensor_f64(G, e->theta, cur, e->sigma, stream))) return rc;
        if ((rc = ins_k_apply_bc_p_fields(G, e->sigma, D * (D + 1) / 2, s))) return rc;
        if ((rc = ins_divoftensor_f64(G, e->sigma, e->E, stream))) return rc;
      }
      if (with_temp && td.dodissipation && !w_from_stage && (rc = ins_k_diffusion_flux3d(G, visc, cur, e->diff, false, s)))
        return rc;  // e->diff: shell zero since its allocation
      RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, RK_K_BASIS, false, RK_FORCE_INDEX_ORDER);  // k-basis only
      epi.ustart = (i == 0) ? nullptr : u;
      epi.ustar = out;
      epi.extra = closure ? e->E : nullptr;
      if (with_temp) {  // gravity inside the stage kernel (two loads of temp per volume)
        epi.gtemp = tin;
        epi.ga2 = td.a2;
        epi.gdir = td.gdir;
        if (w_from_stage) epi.wout = e->w;
      }
      if ((rc = ins_k_momentum_rk_fused(G, visc, cur, rk->ku[i], epi, s))) return rc;
      if (with_temp) {
        double coefs[INS_MAX_STAGES];
        const double* ks[INS_MAX_STAGES];
        int n = 0;
        for (int j = 0; j < i; ++j) {
          coefs[n] = dt * rk->A[i * ns + j];
          ks[n] = e->ktemp[j];
          ++n;
        }
        const bool later = ins_rk_needed_later(rk->A.data(), ns, i);
        if ((rc = ins_k_temp_stage(G, td.a4, td.diss_coef, cur, tin, w_from_stage ? e->w : nullptr, e->tempstart, n, coefs, ks, dt * rk->A[i * ns + i],
                                   later ? e->ktemp[i].get() : nullptr, tout, s, nullptr, td.dodissipation && !w_from_stage ? e->diff.get() : nullptr)))
          return rc;
      }
      if ((rc = ins_k_apply_bc_u(G, out, 0, nullptr, s))) return rc;                                          // :48
      if ((rc = ins_k_project(G, rk->ps, out, rk->p, s))) return rc;                                            // :49
      cur = out;
      tin = tout;
    }
    if (ns == 1) {
      INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], vbytes, hipMemcpyDeviceToDevice, s));
      if (with_temp) INS_HIP_TRY(hipMemcpyAsync(temp, e->tb[0], sbytes, hipMemcpyDeviceToDevice, s));
    }
    if ((rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;                                               // :55
    return bc_temp();                                                                                          // :56
  }

  // any grid: the reference's kernel sequence
  INS_HIP_TRY(hipMemcpyAsync(rk->ustart, u, vbytes, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < ns; ++i) {
    if ((rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;
    if ((rc = bc_temp())) return rc;
    rc = ins_fast3d_supported(G) ? ins_k_momentum_fast3d_opts(G, visc, u, rk->ku[i], false, s) : ins_k_momentum_generic(G, visc, u, rk->ku[i], s);
    if (rc) return rc;
    if (with_temp && (rc = ins_gravity_f64(G, td.gdir, td.a2, temp, rk->ku[i], stream))) return rc;
    if ((rc = temp_rhs(u, i))) return rc;
    if (closure) {
      if ((rc = need_sigma())) return rc;
      if ((rc = ins_smagtensor_f64(G, e->theta, u, e->sigma, stream))) return rc;
      if ((rc = ins_k_apply_bc_p_fields(G, e->sigma, D * (D + 1) / 2, s))) return rc;
      if ((rc = ins_divoftensor_f64(G, e->sigma, e->E, stream))) return rc;
      const double one = 1.0;
      const double* ks[1] = {e->E};
      if ((rc = ins_combine_f64(G, rk->ku[i], rk->ku[i], 1, &one, ks, stream))) return rc;  // ku[i] += m(u, θ)
    }
    double coefs[INS_MAX_STAGES + 1];
    const double* ks[INS_MAX_STAGES + 1];
    const int n = ins_rk_sum_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, coefs, ks);
    if ((rc = ins_combine_f64(G, rk->ustart, u, n, coefs, ks, stream))) return rc;
    if ((rc = temp_combine(i))) return rc;
    if ((rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;
    if ((rc = ins_k_project(G, rk->ps, u, rk->p, s))) return rc;
  }
  if ((rc = ins_k_apply_bc_u(G, u, 0, nullptr, s))) return rc;
  return bc_temp();
}
