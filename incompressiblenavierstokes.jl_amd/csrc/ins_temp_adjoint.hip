// Reverse-mode pullbacks of the temperature equation in fp64 (operators.jl:712-737, 791-814, 884-931; boundary_conditions.jl:236-270, 338-342,
// 391-412, 466-470, 512-516): each is the exact transpose of THIS library's forward operator (ins_fields.hip: k_bc_temp, k_gravity,
// k_convdiff_temp, diffusion + k_dissipation_interp) on the whole padded arrays (DESIGN.md "Differentiability", "Temperature equation").
//
// The kernels are the templates of ins_temp_adjoint_kernels.h with T = double, the ones ins_temp_adjoint32.hip instantiates with float.
// This file holds no stencil arithmetic of its own: the slab refusal and the entry points.
#include "ins_temp_adjoint_kernels.h"

namespace {

// z-slab grids (INS_BC_HALO sides): the ghost planes belong to another rank, whose cotangents this rank does not hold
int refuse_slab(const ins_grid* G, const char* what) {
  for (int b = 0; b < G->g.D; ++b)
    if (G->g.bc[b][0] == INS_BC_HALO || G->g.bc[b][1] == INS_BC_HALO) {
      ins_set_error("%s: slab (halo) grids are not supported", what);
      return INS_ERR_UNSUPPORTED;
    }
  return INS_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// apply_bc_temp_pullback!   boundary_conditions.jl:142-157, 248-270, 341-342, 407-412, 469-470, 515-516 (in place)
extern "C" int ins_apply_bc_temp_pullback_f64(const ins_grid_t* G, const int32_t* bc, double* tempbar, void* stream) {
  INS_REQUIRE(G && bc && tempbar, "null argument");
  int rc;
  if ((rc = refuse_slab(G, "ins_apply_bc_temp_pullback_f64"))) return rc;
  return bc_temp_pullback<double>(G, bc, tempbar, as_stream(stream));
}

// gravity_adjoint!   operators.jl:892-908 (tempbar += ...)
extern "C" int ins_gravity_adjoint_f64(const ins_grid_t* G, int gdir, double a2, const double* phibar, double* tempbar, void* stream) {
  INS_REQUIRE(G && phibar && tempbar, "null argument");
  INS_REQUIRE(gdir >= 0 && gdir < G->g.D, "gravity direction");
  INS_REQUIRE(tempbar != phibar + (long long)gdir * G->g.sc, "gravity_adjoint! cannot run in place");
  int rc;
  if ((rc = refuse_slab(G, "ins_gravity_adjoint_f64"))) return rc;
  TempAdjArgs<double> a{};
  a.gdir = gdir;
  a.a2 = a2;
  a.Fbar = phibar;
  a.tempbar = tempbar;
  return launch_temp_adjoint<double, P_GRAV, false>(G, a, as_stream(stream));
}

// convection_diffusion_temp_adjoint!   operators.jl:712-737 (ubar += ..., tempbar += ...; either may be NULL)
extern "C" int ins_convection_diffusion_temp_adjoint_f64(const ins_grid_t* G, double a4, const double* u, const double* temp, const double* cbar,
                                                         double* ubar, double* tempbar, void* stream) {
  INS_REQUIRE(G && u && temp && cbar, "null argument");
  INS_REQUIRE(ubar || tempbar, "ubar and tempbar are both NULL");
  INS_REQUIRE(tempbar != cbar && tempbar != temp, "convection_diffusion_temp_adjoint! cannot run in place");
  INS_REQUIRE(ubar != u, "convection_diffusion_temp_adjoint! cannot run in place");
  int rc;
  if ((rc = refuse_slab(G, "ins_convection_diffusion_temp_adjoint_f64"))) return rc;
  TempAdjArgs<double> a{};
  a.a4 = a4;
  a.u = u;
  a.temp = temp;
  a.cbar = cbar;
  a.ubar = ubar;
  a.tempbar = tempbar;
  if (ubar && tempbar) return launch_temp_adjoint<double, P_CDT_T | P_CDT_U, false>(G, a, as_stream(stream));
  if (tempbar) return launch_temp_adjoint<double, P_CDT_T, false>(G, a, as_stream(stream));
  return launch_temp_adjoint<double, P_CDT_U, false>(G, a, as_stream(stream));
}

// dissipation_adjoint!   operators.jl:791-814 (ubar += ...)
extern "C" int ins_dissipation_adjoint_f64(const ins_grid_t* G, double visc, double coef, const double* u, const double* cbar, double* ubar,
                                           void* stream) {
  INS_REQUIRE(G && u && cbar && ubar, "null argument");
  INS_REQUIRE(ubar != u, "dissipation_adjoint! cannot run in place");
  int rc;
  if ((rc = refuse_slab(G, "ins_dissipation_adjoint_f64"))) return rc;
  TempAdjArgs<double> a{};
  a.visc = visc;
  a.coef = coef;
  a.u = u;
  a.cbar = cbar;
  a.ubar = ubar;
  return launch_temp_adjoint<double, P_DISS, false>(G, a, as_stream(stream));
}

// One stage's temperature-coupled pullback in one launch   step_explicit_runge_kutta.jl:79-83 (tempbar = ..., ubar += ...)
extern "C" int ins_temperature_pullback_f64(const ins_grid_t* G, const ins_temperature_desc_t* desc, double visc, const double* u, const double* temp,
                                            const double* Fbar, const double* cbar, double* ubar, double* tempbar, void* stream) {
  INS_REQUIRE(G && desc && u && temp && Fbar && cbar && ubar && tempbar, "null argument");
  INS_REQUIRE(desc->gdir >= 0 && desc->gdir < G->g.D, "gravity direction");
  INS_REQUIRE(ubar != u && ubar != Fbar, "temperature pullback cannot run in place");
  INS_REQUIRE(tempbar != temp && tempbar != cbar, "temperature pullback cannot run in place");
  int rc;
  if ((rc = refuse_slab(G, "ins_temperature_pullback_f64"))) return rc;
  TempAdjArgs<double> a{};
  a.gdir = desc->gdir;
  a.a2 = desc->a2;
  a.a4 = desc->a4;
  a.visc = visc;
  a.coef = desc->diss_coef;
  a.u = u;
  a.temp = temp;
  a.Fbar = Fbar;
  a.cbar = cbar;
  a.ubar = ubar;
  a.tempbar = tempbar;
  if (desc->dodissipation) return launch_temp_adjoint<double, P_GRAV | P_CDT_T | P_CDT_U | P_DISS, true>(G, a, as_stream(stream));
  return launch_temp_adjoint<double, P_GRAV | P_CDT_T | P_CDT_U, true>(G, a, as_stream(stream));
}
