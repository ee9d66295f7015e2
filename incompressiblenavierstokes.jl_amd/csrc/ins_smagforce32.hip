// Smagorinsky closure with T = Float32 (operators.jl:1135-1150, 1203-1236, 1284-1305; the reference is generic in T):
//   one kernel     : the float instantiations of ins_smagforce_kernels.h in its three non-correcting forms (uniform periodic, GEN, GEN + STR); the
//                    correcting form is not instantiated — the Float32 extended stage loop (ins_f32.hip) feeds corrected velocities;
//   three kernels  : k_smagtensor<D, float> (ins_tensorbasis.h) -> k_bc_p<D, float> on the D(D+1)/2 stress fields -> ins_divoftensor_f32, for 2-D grids
//                    and the grids ins_smagforce_supported refuses; also the in-device cross-check of the one-kernel form.
// The route predicate is the fp64 one (ins_smagforce.hip), with its switches INS_DISABLE_SMAGFORCE, INS_DISABLE_SMAGFORCE_GEN and INS_SMAGFORCE_ZC.
// The conventions of ins_f32g.hip: float fields in the reference layout, the fp64 grid handle, metric tables rounded to float where they enter, all
// arithmetic in float.  A translation unit of its own so that the fp64 kernels keep their register allocation.  Slab (HALO) sides are not taken.
//
// THIS FILE IS COMPILED WITH -mllvm -amdgpu-dpp-combine=false (csrc/Makefile).  A float wave shift is one v_mov_b32_dpp, and the compiler's DPP-combine
// pass folds some of them into the arithmetic that consumes them (v_add_f32_dpp / v_subrev_f32_dpp; a double shift is two moves and is never folded, so
// the fp64 file is not concerned).  With the folding the GEN + STR float form returned values off by 4e-4 .. 6e-3 of max|s| on an MI355X — on the second
// output row of a wavefront's row pair, mostly one plane in four — while the uniform and GEN float forms were right; without it the same source is right to
// 1.7e-7 (profiles/smagforce_generic_isa.md: the 19 folded instructions, all in full-EXEC regions; which fold is at fault is not identified).
#include "ins_f32_internal.h"
#include "ins_smagforce_kernels.h"
#include "ins_tensorbasis.h"

// s (degrees of freedom of the three components; everything else untouched) = closure force of the velocity field u with its boundary data applied
// (periodic directions: ghost volumes not read)
int ins_k_smagforce_f32(const ins_grid* G, float theta, const float* u, float* sout, hipStream_t s) {
  const int force = (int)ins_opt(OPT_INS_SMAGFORCE_FORCE_GEN);  // experiment: the generalised forms on a periodic uniform box (1: uniform, 2: stretched)
  const bool gen = !smagforce_uniform(G) || force;
  if (!ins_smagforce_supported(G)) {
    ins_set_error("ins_k_smagforce_f32: grid not supported");
    return INS_ERR_UNSUPPORTED;
  }
  constexpr int R = SF_R;
  SmagArgs<float> a;
  const unsigned nb = smagforce_args<float>(G, theta, u, nullptr, sout, a);
  if (gen && (!G->uniform_exact || force == 2))
    hipLaunchKernelGGL((k_smagforce<float, R, false, true, true>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  else if (gen)
    hipLaunchKernelGGL((k_smagforce<float, R, false, true, false>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  else
    hipLaunchKernelGGL((k_smagforce<float, R, false>), dim3(nb), dim3(64, 4, 1), 0, s, a);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

extern "C" int ins_smagtensor_f32(const ins_grid_t* G, float theta, const float* u, float* sigma, void* stream) {
  INS_REQUIRE(G && u && sigma, "null argument");
  int rc = no_halo(G, "smagtensor (f32)");
  if (rc) return rc;
  INS_REQUIRE(sigma != u, "smagtensor! cannot run in place");
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_smagtensor<D, float>), box_launch(g.D, g.ip_lo, g.ip_hi), as_stream(stream), g, theta, u, sigma);
  return INS_OK;
}

extern "C" int ins_smagorinsky_force_f32(const ins_grid_t* G, float theta, const float* u, float* sigma, float* s, void* stream) {
  INS_REQUIRE(G && u && s, "null argument");
  int rc = no_halo(G, "smagorinsky_force (f32)");  // (fp64 too: the stress tensor's ghost planes would have to travel between the ranks inside this call)
  if (rc) return rc;
  if (ins_smagforce_supported(G)) return ins_k_smagforce_f32(G, theta, u, s, as_stream(stream));
  INS_REQUIRE(sigma, "sigma scratch needed on this grid");
  const int D = G->g.D;
  if ((rc = ins_smagtensor_f32(G, theta, u, sigma, stream))) return rc;
  if ((rc = ins_k32g_apply_bc_p_fields(G, sigma, D * (D + 1) / 2, as_stream(stream)))) return rc;
  return ins_divoftensor_f32(G, sigma, s, stream);
}
