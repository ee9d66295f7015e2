// Pullback of the Smagorinsky closure force with T = Float32: the float instantiations of ins_smagpullback_kernels.h.  The conventions of
// ins_tensorclosure32.hip: float fields in the reference layout, the fp64 grid handle, metric tables rounded to float where they enter, all arithmetic in
// float; the ∇ubar scratch is the grid handle's, its first half used as D·D floats per volume.  The cell's term of <σ̄, σ̂> is formed in float and
// summed in double, and θbar is a device double, as in fp64.  A translation unit of its own so that the fp64 kernels keep their register allocation.
#include "ins_f32_internal.h"
#include "ins_smagpullback_kernels.h"

extern "C" int ins_smagorinsky_force_pullback_f32(const ins_grid_t* G, float theta, const float* u, const float* sbar, float* ubar, int accumulate,
                                                  double* thetabar, void* stream) {
  INS_REQUIRE(G && u && sbar && ubar, "null argument");
  if (int rc = no_halo(G, "smagorinsky_force pullback (f32)")) return rc;
  INS_REQUIRE(ubar != u && ubar != sbar, "the Smagorinsky force pullback cannot run in place (ubar aliases u or sbar)");
  INS_REQUIRE((const void*)thetabar != (const void*)u && (const void*)thetabar != (const void*)sbar && (const void*)thetabar != (const void*)ubar,
              "thetabar aliases a field");
  hipStream_t s = as_stream(stream);
  double *gb64 = nullptr, *part = nullptr;
  int rc;
  if ((rc = ins_k_gradbar_scratch(G, &gb64))) return rc;
  if (thetabar && (rc = ins_k_smag_partials(G, &part))) return rc;
  float* gb = reinterpret_cast<float*>(gb64);
  if ((rc = launch_smag_gradbar<float>(G, theta, u, sbar, gb, part, thetabar, s))) return rc;
  return ins_k32_gradu_adjoint(G, gb, ubar, accumulate != 0, s);
}
