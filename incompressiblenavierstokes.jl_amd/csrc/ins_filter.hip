// DNS-to-LES filters of lib/NeuralClosure (filter.jl), fp64: the double instantiations of ins_filter_kernels.h behind the _f64 entries
// (DESIGN.md §6c).  The tiled kernel keeps one fine x-volume (8 B) per lane.
#include "ins_filter_kernels.h"

extern "C" int ins_filter_face_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, const double* u, double* v, void* stream) {
  return launch_filter<false, double, 1>(les, dns, comp, u, v, as_stream(stream));
}

extern "C" int ins_filter_volume_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, const double* u, double* v, void* stream) {
  return launch_filter<true, double, 1>(les, dns, comp, u, v, as_stream(stream));
}

// The two filters for the nbatch members of an ensemble of 2-D fields in one launch (member on blockIdx.z): the window sums are the text of k_filter<2, VOL, double>,
// so member b is bitwise what the entries above give for that field alone.
extern "C" int ins_filter_face_members_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, int nbatch, const double* u, int64_t ustride, double* v,
                                           int64_t vstride, void* stream) {
  return launch_filter_members<false, double>(les, dns, comp, nbatch, u, ustride, v, vstride, as_stream(stream));
}

extern "C" int ins_filter_volume_members_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, int nbatch, const double* u, int64_t ustride, double* v,
                                             int64_t vstride, void* stream) {
  return launch_filter_members<true, double>(les, dns, comp, nbatch, u, ustride, v, vstride, as_stream(stream));
}

extern "C" int ins_reconstruct_f64(const ins_grid_t* dns, const ins_grid_t* les, int comp, const double* v, double* u, void* stream) {
  return launch_reconstruct<double>(dns, les, comp, v, u, as_stream(stream));
}

extern "C" int ins_filter_face_pullback_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, const double* w, double* ubar, void* stream) {
  return launch_filter_pullback<false, double>(les, dns, comp, w, ubar, as_stream(stream));
}

extern "C" int ins_filter_volume_pullback_f64(const ins_grid_t* les, const ins_grid_t* dns, int comp, const double* w, double* ubar, void* stream) {
  return launch_filter_pullback<true, double>(les, dns, comp, w, ubar, as_stream(stream));
}
