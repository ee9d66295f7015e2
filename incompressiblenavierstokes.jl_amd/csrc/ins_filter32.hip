// DNS-to-LES filters of lib/NeuralClosure (filter.jl) with T = Float32: the float instantiations of ins_filter_kernels.h behind the _f32 entries
// (DESIGN.md §6c "Float32").  float loads and stores, double accumulation, one rounding at the store.  The conventions of ins_f32g.hip: float
// fields in the reference layout, the fp64 grid handles.  A translation unit of its own so that the fp64 kernels keep their register allocation.
// Slab (HALO) sides are not taken.
#include "ins_filter_kernels.h"

namespace {

// fine x-volumes per lane of the tiled kernel: a wavefront's row segment is 64·W·4 bytes
constexpr int FILTER32_W = 2;

int no_halo2(const ins_grid* les, const ins_grid* dns, const char* what) {
  INS_REQUIRE(les && dns, "null grid handle");
  int rc = no_halo(les, what);
  return rc ? rc : no_halo(dns, what);
}

}  // namespace

extern "C" int ins_filter_face_f32(const ins_grid_t* les, const ins_grid_t* dns, int comp, const float* u, float* v, void* stream) {
  int rc = no_halo2(les, dns, "filter_face (f32)");
  return rc ? rc : launch_filter<false, float, FILTER32_W>(les, dns, comp, u, v, as_stream(stream));
}

extern "C" int ins_filter_volume_f32(const ins_grid_t* les, const ins_grid_t* dns, int comp, const float* u, float* v, void* stream) {
  int rc = no_halo2(les, dns, "filter_volume (f32)");
  return rc ? rc : launch_filter<true, float, FILTER32_W>(les, dns, comp, u, v, as_stream(stream));
}

extern "C" int ins_reconstruct_f32(const ins_grid_t* dns, const ins_grid_t* les, int comp, const float* v, float* u, void* stream) {
  int rc = no_halo2(les, dns, "reconstruct (f32)");
  return rc ? rc : launch_reconstruct<float>(dns, les, comp, v, u, as_stream(stream));
}

extern "C" int ins_filter_face_pullback_f32(const ins_grid_t* les, const ins_grid_t* dns, int comp, const float* w, float* ubar, void* stream) {
  int rc = no_halo2(les, dns, "filter_face_pullback (f32)");
  return rc ? rc : launch_filter_pullback<false, float>(les, dns, comp, w, ubar, as_stream(stream));
}

extern "C" int ins_filter_volume_pullback_f32(const ins_grid_t* les, const ins_grid_t* dns, int comp, const float* w, float* ubar, void* stream) {
  int rc = no_halo2(les, dns, "filter_volume_pullback (f32)");
  return rc ? rc : launch_filter_pullback<true, float>(les, dns, comp, w, ubar, as_stream(stream));
}
