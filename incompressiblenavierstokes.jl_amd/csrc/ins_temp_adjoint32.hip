// Reverse-mode pullbacks of the temperature equation of the `_f32` family (operators.jl:712-737, 791-814, 884-931; boundary_conditions.jl:236-270,
// 338-342, 391-412, 466-470, 512-516): each the exact transpose of the `_f32` forward operator (csrc/ins_temp32.hip: k_bc_temp, k_gravity,
// k32t_convdiff_temp, k32t_diffusion + k_dissipation_interp) on the whole padded arrays, ghost volumes included (DESIGN.md "Differentiability").
//
// The kernels are the templates of ins_temp_adjoint_kernels.h with T = float, the ones ins_temp_adjoint.hip instantiates with double: float
// fields in the reference layout, the fp64 grid handle, metric tables read as doubles and rounded to float where they enter the arithmetic,
// arithmetic in float (the conventions of ins_temp32.hip).  This file holds no stencil arithmetic of its own: the entry points, with the
// argument order, the += / overwrite rules, the aliasing checks and the BC-code checks of their `_f64` namesakes.  A translation unit of
// its own so that the fp64 kernels keep their register allocation (ins_stencil.h).  Slab (HALO) sides are not taken: the multi-GPU path is fp64.
#include "ins_temp_adjoint_kernels.h"

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// apply_bc_temp_pullback!   boundary_conditions.jl:142-157, 248-270, 341-342, 407-412, 469-470, 515-516 (in place)
extern "C" int ins_apply_bc_temp_pullback_f32(const ins_grid_t* G, const int32_t* bc, float* tempbar, void* stream) {
  INS_REQUIRE(G && bc && tempbar, "null argument");
  int rc = no_halo(G, "ins_apply_bc_temp_pullback_f32");
  if (rc) return rc;
  return bc_temp_pullback<float>(G, bc, tempbar, as_stream(stream));
}

// gravity_adjoint!   operators.jl:892-908 (tempbar += ...)
extern "C" int ins_gravity_adjoint_f32(const ins_grid_t* G, int gdir, float a2, const float* phibar, float* tempbar, void* stream) {
  INS_REQUIRE(G && phibar && tempbar, "null argument");
  INS_REQUIRE(gdir >= 0 && gdir < G->g.D, "gravity direction");
  INS_REQUIRE(tempbar != phibar + (long long)gdir * G->g.sc, "gravity_adjoint! cannot run in place");
  int rc = no_halo(G, "ins_gravity_adjoint_f32");
  if (rc) return rc;
  TempAdjArgs<float> a{};
  a.gdir = gdir;
  a.a2 = a2;
  a.Fbar = phibar;
  a.tempbar = tempbar;
  return launch_temp_adjoint<float, P_GRAV, false>(G, a, as_stream(stream));
}

// convection_diffusion_temp_adjoint!   operators.jl:712-737 (ubar += ..., tempbar += ...; either may be NULL)
extern "C" int ins_convection_diffusion_temp_adjoint_f32(const ins_grid_t* G, float a4, const float* u, const float* temp, const float* cbar,
                                                         float* ubar, float* tempbar, void* stream) {
  INS_REQUIRE(G && u && temp && cbar, "null argument");
  INS_REQUIRE(ubar || tempbar, "ubar and tempbar are both NULL");
  INS_REQUIRE(tempbar != cbar && tempbar != temp, "convection_diffusion_temp_adjoint! cannot run in place");
  INS_REQUIRE(ubar != u, "convection_diffusion_temp_adjoint! cannot run in place");
  int rc = no_halo(G, "ins_convection_diffusion_temp_adjoint_f32");
  if (rc) return rc;
  TempAdjArgs<float> a{};
  a.a4 = a4;
  a.u = u;
  a.temp = temp;
  a.cbar = cbar;
  a.ubar = ubar;
  a.tempbar = tempbar;
  if (ubar && tempbar) return launch_temp_adjoint<float, P_CDT_T | P_CDT_U, false>(G, a, as_stream(stream));
  if (tempbar) return launch_temp_adjoint<float, P_CDT_T, false>(G, a, as_stream(stream));
  return launch_temp_adjoint<float, P_CDT_U, false>(G, a, as_stream(stream));
}

// dissipation_adjoint!   operators.jl:791-814 (ubar += ...)
extern "C" int ins_dissipation_adjoint_f32(const ins_grid_t* G, float visc, float coef, const float* u, const float* cbar, float* ubar,
                                           void* stream) {
  INS_REQUIRE(G && u && cbar && ubar, "null argument");
  INS_REQUIRE(ubar != u, "dissipation_adjoint! cannot run in place");
  int rc = no_halo(G, "ins_dissipation_adjoint_f32");
  if (rc) return rc;
  TempAdjArgs<float> a{};
  a.visc = visc;
  a.coef = coef;
  a.u = u;
  a.cbar = cbar;
  a.ubar = ubar;
  return launch_temp_adjoint<float, P_DISS, false>(G, a, as_stream(stream));
}

// One stage's temperature-coupled pullback in one launch   step_explicit_runge_kutta.jl:79-83 (tempbar = ..., ubar += ...)
extern "C" int ins_temperature_pullback_f32(const ins_grid_t* G, const ins_temperature_desc_t* desc, float visc, const float* u, const float* temp,
                                            const float* Fbar, const float* cbar, float* ubar, float* tempbar, void* stream) {
  INS_REQUIRE(G && desc && u && temp && Fbar && cbar && ubar && tempbar, "null argument");
  INS_REQUIRE(desc->gdir >= 0 && desc->gdir < G->g.D, "gravity direction");
  INS_REQUIRE(ubar != u && ubar != Fbar, "temperature pullback cannot run in place");
  INS_REQUIRE(tempbar != temp && tempbar != cbar, "temperature pullback cannot run in place");
  int rc = no_halo(G, "ins_temperature_pullback_f32");
  if (rc) return rc;
  TempAdjArgs<float> a{};
  a.gdir = desc->gdir;
  a.a2 = (float)desc->a2;  // rounded once, as ins_rk_step_ext_f32 rounds the descriptor's scalars
  a.a4 = (float)desc->a4;
  a.visc = visc;
  a.coef = (float)desc->diss_coef;
  a.u = u;
  a.temp = temp;
  a.Fbar = Fbar;
  a.cbar = cbar;
  a.ubar = ubar;
  a.tempbar = tempbar;
  if (desc->dodissipation) return launch_temp_adjoint<float, P_GRAV | P_CDT_T | P_CDT_U | P_DISS, true>(G, a, as_stream(stream));
  return launch_temp_adjoint<float, P_GRAV | P_CDT_T | P_CDT_U, true>(G, a, as_stream(stream));
}
