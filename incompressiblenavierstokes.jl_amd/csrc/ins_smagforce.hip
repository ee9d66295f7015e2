// Smagorinsky closure force in one pass, fp64: the double instantiations of ins_smagforce_kernels.h (which describes the kernel), the route
// predicate for both precisions, the launcher and the fp64 entry points.  The Float32 twin is ins_smagforce32.hip.
#include "ins_smagforce_kernels.h"

bool ins_smagforce_supported(const ins_grid* G) {
  const GridDev& g = G->g;
  if (ins_opt(OPT_INS_DISABLE_SMAGFORCE) || g.D != 3 || g.N[0] - 2 < 4 || g.N[1] - 2 < 4 || g.N[2] - 2 < 4) return false;
  if (smagforce_uniform(G)) return true;
  if (ins_opt(OPT_INS_DISABLE_SMAGFORCE_GEN)) return false;
  for (int d = 0; d < 3; ++d)
    for (int side = 0; side < 2; ++side)
      // a PressureBC on the RIGHT side is a zero ghost stress (apply_bc_p!: p[I] .= 0, boundary_conditions.jl:497-501) with one more degree of freedom of the
      // normal component (the masks come from the grid's Iu); on the LEFT side it adds a second ghost layer (N = n + 3), which this kernel's indexing does
      // not cover: the three kernels.  Slab grids: refused by the entry points.
      if ((g.bc[d][side] == INS_BC_PRESSURE && side == 0) || g.bc[d][side] == INS_BC_HALO) return false;
  return true;
}

// s (degrees of freedom of the three components; everything else untouched) = closure force of u.  pI == nullptr: u is a velocity field with its
// boundary data applied (periodic directions: ghost volumes not read); else (all-periodic uniform boxes) u is an uncorrected stage velocity and
// pI the (unpadded) pressure of its projection.
int ins_k_smagforce(const ins_grid* G, double theta, const double* u, const double* pI, double* sout, hipStream_t s) {
  const int force = (int)ins_opt(OPT_INS_SMAGFORCE_FORCE_GEN);  // experiment: the generalised forms on a periodic uniform box (1: uniform, 2: stretched)
  const bool gen = !smagforce_uniform(G) || (force && !pI);
  if (!ins_smagforce_supported(G) || (gen && pI)) {
    ins_set_error("ins_k_smagforce: grid not supported");
    return INS_ERR_UNSUPPORTED;
  }
  constexpr int R = SF_R;
  SmagArgs<double> a;
  const unsigned nb = smagforce_args<double>(G, theta, u, pI, sout, a);
  if (gen && (!G->uniform_exact || force == 2))  // (uniform_exact: every width and every centre distance incl. the ghost layers equal to 2.5e-13)
    hipLaunchKernelGGL((k_smagforce<double, R, false, true, true>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  else if (gen)  // uniform spacing with walls: the central-difference form, ghost rules and masks only
    hipLaunchKernelGGL((k_smagforce<double, R, false, true, false>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  else if (pI)
    hipLaunchKernelGGL((k_smagforce<double, R, true>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  else
    hipLaunchKernelGGL((k_smagforce<double, R, false>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// smagorinsky_closure(setup)(u, θ)   operators.jl:1284-1300 as one kernel where the box allows it, else the reference's three steps
// (sigma: scratch of D(D+1)/2 scalar fields, used by the three-step route only)
extern "C" int ins_smagorinsky_force_needs_sigma(const ins_grid_t* G) { return (G && ins_smagforce_supported(G)) ? 0 : 1; }
extern "C" int ins_smagorinsky_force_f64(const ins_grid_t* G, double theta, const double* u, double* sigma, double* s, void* stream) {
  INS_REQUIRE(G && u && s, "null argument");
  if (has_halo_side(G)) {  // the stress tensor's ghost planes would have to travel between the ranks inside this call
    ins_set_error("ins_smagorinsky_force_f64: z-slab grids (INS_BC_HALO sides) are not supported");
    return INS_ERR_UNSUPPORTED;
  }
  if (ins_smagforce_supported(G)) return ins_k_smagforce(G, theta, u, nullptr, s, as_stream(stream));
  INS_REQUIRE(sigma, "sigma scratch needed on this grid");
  const int D = G->g.D;
  int rc;
  if ((rc = ins_smagtensor_f64(G, theta, u, sigma, stream))) return rc;
  if ((rc = ins_k_apply_bc_p_fields(G, sigma, D * (D + 1) / 2, as_stream(stream)))) return rc;
  return ins_divoftensor_f64(G, sigma, s, stream);
}
