// Reverse-mode pullbacks of the `_f32` family (operators.jl:100-616, boundary_conditions.jl:114-230, 290-516, pressure.jl:15-19, 52-82):
// each the exact transpose of the `_f32` forward operator (csrc/ins_f32.hip, ins_f32g.hip) on the whole padded array, ghost volumes
// included (DESIGN.md "Differentiability").
//
// The kernels are the templates of ins_adjoint_kernels.h with T = float, the ones ins_adjoint.hip instantiates with double: float fields in
// the reference layout, the fp64 grid handle, metric tables read as doubles and rounded to float where they enter the arithmetic,
// arithmetic in float (the conventions of ins_f32g.hip).  This file holds no stencil arithmetic of its own: the instantiations, the ghost
// zeroing and the host logic of the projection pullback, and the entry points.  A translation unit of its own so that the fp64 kernels keep
// their register allocation (ins_stencil.h).  Slab (HALO) sides are not taken: the multi-GPU path is fp64.
#include "ins_adjoint_kernels.h"
#include "ins_f32_internal.h"

namespace {

// Z of the spectral projection pullback: the two ghost planes of direction be of a vector field are set to zero (periodic boxes)
template <int D>
__global__ __launch_bounds__(256) void k32a_zero_ghosts(GridDev g, float* __restrict__ u, int be) {
  INS_LINE_INDEX(be);
  float* ua = u + blockIdx.z * g.sc + base;
  ua[(g.ip_lo[be] - 1) * g.sx[be]] = 0.f;
  ua[g.ip_hi[be] * g.sx[be]] = 0.f;
}

int bc_u_pullback32(const ins_grid* G, float* u, hipStream_t s) {
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k32g_apply_bc_u
    INS_LAUNCH_D((k_bc_u_pullback<D, float>), line_launch(g, be, g.D), s, g, u, be);
  }
  return INS_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_divergence_adjoint_f32(const ins_grid_t* G, const float* phi, float* ubar, void* stream) {
  INS_REQUIRE(G && phi && ubar, "null argument");
  int rc = no_halo(G, "divergence_adjoint (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_divergence_adjoint<D, float, float>), box_launch(g.D, g.N), as_stream(stream), g, phi, ubar, 1.f);
  return INS_OK;
}

extern "C" int ins_pressuregradient_adjoint_f32(const ins_grid_t* G, const float* phi, float* pbar, void* stream) {
  INS_REQUIRE(G && phi && pbar, "null argument");
  int rc = no_halo(G, "pressuregradient_adjoint (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_pressuregradient_adjoint<D, float, float, true>), box_launch(g.D, g.N), as_stream(stream), g, phi, pbar);
  return INS_OK;
}

extern "C" int ins_momentum_pullback_f32(const ins_grid_t* G, float visc, const float* u, const float* phibar, float* ubar, int accumulate,
                                         void* stream) {
  INS_REQUIRE(G && u && phibar && ubar, "null argument");
  INS_REQUIRE(ubar != u && ubar != phibar, "momentum pullback cannot run in place");
  int rc = no_halo(G, "momentum pullback (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  if (accumulate)
    INS_LAUNCH_D((k_convdiff_adjoint<D, float, 3, true>), l, as_stream(stream), g, visc, u, phibar, ubar);
  else
    INS_LAUNCH_D((k_convdiff_adjoint<D, float, 3, false>), l, as_stream(stream), g, visc, u, phibar, ubar);
  return INS_OK;
}

extern "C" int ins_apply_bc_u_pullback_f32(const ins_grid_t* G, float* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  int rc = no_halo(G, "apply_bc_u pullback (f32)");
  if (rc) return rc;
  return bc_u_pullback32(G, phibar, as_stream(stream));
}

extern "C" int ins_apply_bc_p_pullback_f32(const ins_grid_t* G, float* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  int rc = no_halo(G, "apply_bc_p pullback (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k32g_apply_bc_p
    if (g.bc[be][0] == INS_BC_DIRICHLET && g.bc[be][1] == INS_BC_DIRICHLET) continue;
    INS_LAUNCH_D((k_bc_p_pullback<D, float>), line_launch(g, be, 1), as_stream(stream), g, phibar, be);
  }
  return INS_OK;
}

// Wrapped solver: ins_k32g_project is u ↦ u − G·bc_p(round(poisson(Ω·D u))) on the DOF volumes with D u taken in double from the float field
// (left ghost column included) and every other volume left alone, so φ ← φ − round(Dᵀ·Ω·poisson·bc_pᵀ·Gᵀ·φ) with everything between Gᵀ and
// Dᵀ in double: the order of ins_project_pullback_f64 (Gᵀ, bc_pᵀ, solve, Ω, −Dᵀ) on the solver's fp64 scratch.
// Spectral solver: ins_project_f32 is u ↦ B·P·Z·u on a uniform periodic box (Z: the ghost values are not read, periodic images are; P: the
// projection of the interior; B: the periodic ghost fill of the result).  There G = −Dᵀ and Ω is a constant, so P = I − G·poisson·Ω·D is
// symmetric and the transpose is Z·P·Bᵀ: the ghost-fill pullback, the forward entry itself (the same solver route, so the same accuracy),
// and the ghosts set to zero.
extern "C" int ins_project_pullback_f32(const ins_grid_t* G, ins_poisson32_t* ps, float* phibar, float* pwork, void* stream) {
  INS_REQUIRE(G && ps && phibar && pwork, "null argument");
  INS_REQUIRE(ins_k32_solver_grid(ps) == G, "psolver was created for a different grid");
  INS_REQUIRE(phibar != pwork, "pwork must be its own array");
  int rc = no_halo(G, "project pullback (f32)");
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  const GridDev& g = G->g;
  double* p64 = nullptr;
  ins_poisson* ps64 = ins_k32_wrapped(ps, &p64);
  if (ps64) {
    if (ps64->kind == POISSON_SPECTRAL && G->all_periodic) {
      ins_set_error("project pullback (f32): a wrapped spectral solver on an all-periodic box is not taken (use ins_poisson_spectral_create_f32)");
      return INS_ERR_UNSUPPORTED;
    }
    INS_LAUNCH_D((k_pressuregradient_adjoint<D, float, double, false>), box_launch(g.D, g.N), s, g, phibar, p64);
    if ((rc = ins_k_apply_bc_p_pullback(G, p64, s))) return rc;
    if ((rc = ins_k_poisson_solve(ps64, p64, s))) return rc;
    if ((rc = ins_k_scalewithvolume(G, p64, s))) return rc;
    INS_LAUNCH_D((k_divergence_adjoint<D, double, float>), box_launch(g.D, g.N), s, g, p64, phibar, -1.0);
    // the forward rounds the whole scratch into its p: leave the volumes outside Ip as ins_poisson_wrap_f32 made them
    INS_HIP_TRY(hipMemsetAsync(p64, 0, G->ncell * sizeof(double), s));
    return INS_OK;
  }
  if ((rc = bc_u_pullback32(G, phibar, s))) return rc;
  if ((rc = ins_project_f32(G, ps, phibar, pwork, stream))) return rc;
  for (int be = 0; be < g.D; ++be) {
    INS_LAUNCH_D((k32a_zero_ghosts<D>), line_launch(g, be, g.D), s, g, phibar, be);
  }
  return INS_OK;
}
