// Pullback of the Smagorinsky closure force, fp64: the double instantiations of ins_smagpullback_kernels.h (which derives the kernels), the
// workgroup-partial scratch of the grid handle for both precisions, and the fp64 entry point.  The Float32 twin is ins_smagpullback32.hip.
#include "ins_smagpullback_kernels.h"

// the grid handle's scratch for the workgroup partials of <σ̄, σ̂>: one double per workgroup of pass 1, allocated and grown on demand (all pullbacks of
// one grid run on one stream at a time, as for the ∇ubar scratch)
int ins_k_smag_partials(const ins_grid* G, double** out) {
  ins_grid* M = const_cast<ins_grid*>(G);
  const size_t need = (size_t)smag_partials(box_launch(G->g.D, G->g.ip_lo, G->g.ip_hi));
  if (int rc = M->smagpart_dev.ensure(need)) return rc;
  *out = M->smagpart_dev;
  return INS_OK;
}

extern "C" int ins_smagorinsky_force_pullback_f64(const ins_grid_t* G, double theta, const double* u, const double* sbar, double* ubar, int accumulate,
                                                  double* thetabar, void* stream) {
  INS_REQUIRE(G && u && sbar && ubar, "null argument");
  if (int rc = no_halo(G, "smagorinsky_force pullback", "slab (INS_BC_HALO) grids are not supported")) return rc;
  INS_REQUIRE(ubar != u && ubar != sbar, "the Smagorinsky force pullback cannot run in place (ubar aliases u or sbar)");
  INS_REQUIRE((const void*)thetabar != (const void*)u && (const void*)thetabar != (const void*)sbar && thetabar != ubar, "thetabar aliases a field");
  hipStream_t s = as_stream(stream);
  double *gb = nullptr, *part = nullptr;
  int rc;
  if ((rc = ins_k_gradbar_scratch(G, &gb))) return rc;
  if (thetabar && (rc = ins_k_smag_partials(G, &part))) return rc;
  if ((rc = launch_smag_gradbar<double>(G, theta, u, sbar, gb, part, thetabar, s))) return rc;
  return ins_k_gradu_adjoint(G, gb, ubar, accumulate != 0, s);
}
