// What the Float32 driver needs besides the step (solver.jl:18-125, processors.jl:78-197 with T = Float32; the reference is generic in T):
//   observers : the float instantiations of ins_fields_kernels.h behind ins_vorticity_f32, ins_interpolate_u_p_f32, ins_interpolate_w_p_f32 and
//               ins_qfield_f32 — the launches of their fp64 namesakes (ins_fields.hip);
//   CFL       : ins_cfl_timestep_f32, get_cfl_timestep! (solver.jl:101-125) as ONE pass over u and a one-workgroup finish, where the fp64 entry
//               writes a cell-sized buffer and reduces it once per direction.
// The conventions of ins_f32g.hip: float fields in the reference layout, the fp64 grid handle, metric tables rounded to float where they enter, all
// arithmetic in float.  A translation unit of its own so that the fp64 kernels keep their register allocation.  Slab (HALO) sides are not taken.
#include "ins_fields_kernels.h"

namespace {

__device__ __forceinline__ float wave_min(float v) {  // minimum over the 64 lanes, in every lane
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}
// minimum over the four wavefronts of a 256-work-item workgroup; valid in work-item 0
__device__ __forceinline__ float block_min(float v, float (&red)[4], int lane, int wave) {
  v = wave_min(v);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// min over α and I ∈ Iu[α] of Δu[α][I_α] / |u_α[I]|                                  solver.jl:115-118
// A wavefront takes whole rows (j, k) of the padded array, its lanes run along x; the rows are dealt to the wavefronts of the launch round-robin.
// A value is loaded only where I ∈ Iu[α] (grid creation keeps Iu inside the array, ins_stencil.h): ghost volumes and faces outside Iu are never
// read, and a direction without faces reads nothing.  u = 0 gives +inf, which the minimum keeps.  One partial per workgroup, plain stores.
constexpr int CFL_MAX_WG = 2048;
template <int D>
__global__ __launch_bounds__(256) void k_cfl32(GridDev g, const float* __restrict__ u, long long nrows, float* __restrict__ partial) {
  __shared__ float red[4];
  const int lane = threadIdx.x, wave = threadIdx.y;
  float m = INFINITY;
  for (long long r = (long long)blockIdx.x * 4 + wave; r < nrows; r += (long long)gridDim.x * 4) {
    const int j = (int)(r % g.N[1]), k = (int)(r / g.N[1]);  // 2-D: nrows = N[1], k = 0
    const long long base = j * g.sx[1] + (D == 3 ? k * g.sx[2] : 0);
    bool row_in[D];
    float d_row[D];  // Δu[α] of the row for α != 0
#pragma unroll
    for (int a = 0; a < D; ++a) {
      row_in[a] = j >= g.iu_lo[a][1] && j < g.iu_hi[a][1] && (D == 2 || (k >= g.iu_lo[a][2] && k < g.iu_hi[a][2]));
      d_row[a] = row_in[a] && a > 0 ? (float)g.dxu[a][a == 1 ? j : k] : 0.f;
    }
    for (int i = lane; i < g.N[0]; i += 64) {
#pragma unroll
      for (int a = 0; a < D; ++a) {
        if (row_in[a] && i >= g.iu_lo[a][0] && i < g.iu_hi[a][0]) {
          const float d = a == 0 ? (float)g.dxu[0][i] : d_row[a];
          m = fminf(m, d / fabsf(u[a * g.sc + base + i]));
        }
      }
    }
  }
  m = block_min(m, red, lane, wave);
  if (lane == 0 && wave == 0) partial[blockIdx.x] = m;
}

__global__ __launch_bounds__(256) void k_cfl32_finish(const float* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float m = INFINITY;
  for (int q = threadIdx.x; q < n; q += 256) m = fminf(m, partial[q]);
  m = block_min(m, red, threadIdx.x & 63, threadIdx.x >> 6);
  if (threadIdx.x == 0) out[0] = m;
}

}  // namespace

extern "C" int ins_cfl_timestep_f32(const ins_grid_t* G, float Re, const float* u, float* out, void* stream) {
  INS_REQUIRE(G && u && out, "null argument");
  int rc = no_halo(G, "cfl_timestep (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  hipStream_t s = as_stream(stream);
  // diffusive bound Re·min(Δu[α])²/2 over α, on the host in double                                      solver.jl:107-113
  double dt_diff = INFINITY;
  for (int a = 0; a < g.D; ++a) {
    double damin = INFINITY;
    for (int i = g.iu_lo[a][a]; i < g.iu_hi[a][a]; ++i) damin = fmin(damin, G->desc.dxu[a][i]);
    dt_diff = fmin(dt_diff, (double)Re * damin * damin / 2);
  }
  // the grid's reduction scratch (4096 doubles on the device, pinned on the host) holds the workgroup partials and, behind them, the result
  float* partial = reinterpret_cast<float*>(G->red_dev.get());
  const long long nrows = (long long)g.N[1] * (g.D == 3 ? g.N[2] : 1);
  const int nwg = (int)std::min<long long>((nrows + 3) / 4, CFL_MAX_WG);
  if (g.D == 2)
    hipLaunchKernelGGL(k_cfl32<2>, dim3(nwg), dim3(64, 4, 1), 0, s, g, u, nrows, partial);
  else
    hipLaunchKernelGGL(k_cfl32<3>, dim3(nwg), dim3(64, 4, 1), 0, s, g, u, nrows, partial);
  INS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cfl32_finish, dim3(1), dim3(256), 0, s, (const float*)partial, nwg, partial + CFL_MAX_WG);
  INS_LAUNCH_CHECK();
  float* host = reinterpret_cast<float*>(G->red_host.get());
  INS_HIP_TRY(hipMemcpyAsync(host, partial + CFL_MAX_WG, sizeof(float), hipMemcpyDeviceToHost, s));
  INS_HIP_TRY(hipStreamSynchronize(s));
  *out = (float)fmin(dt_diff, (double)host[0]);
  return INS_OK;
}

extern "C" int ins_vorticity_f32(const ins_grid_t* G, const float* u, float* w, void* stream) {
  INS_REQUIRE(G && u && w, "null argument");
  int rc = no_halo(G, "vorticity (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  const int hi[3] = {g.N[0] - 1, g.N[1] - 1, g.N[2] - 1};
  Launch3 l = banded_launch(g.D, hi);
  INS_LAUNCH_D((k_vorticity<D, float>), l, as_stream(stream), g, l.map, u, w);
  return INS_OK;
}

extern "C" int ins_interpolate_u_p_f32(const ins_grid_t* G, const float* u, float* up, void* stream) {
  INS_REQUIRE(G && u && up, "null argument");
  int rc = no_halo(G, "interpolate_u_p (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  Launch3 l = banded_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_interp_u_p<D, float>), l, as_stream(stream), g, l.map, u, up);
  return INS_OK;
}

extern "C" int ins_interpolate_w_p_f32(const ins_grid_t* G, const float* w, float* wp, void* stream) {
  INS_REQUIRE(G && w && wp, "null argument");
  int rc = no_halo(G, "interpolate_w_p (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  Launch3 l = banded_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_interp_w_p<D, float>), l, as_stream(stream), g, l.map, w, wp);
  return INS_OK;
}

extern "C" int ins_qfield_f32(const ins_grid_t* G, const float* u, float* Q, void* stream) {
  INS_REQUIRE(G && u && Q, "null argument");
  int rc = no_halo(G, "Qfield (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  Launch3 l = banded_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_Qfield<D, float>), l, as_stream(stream), g, l.map, u, Q);
  return INS_OK;
}
