// Scaffolding of the generic stencil kernels (ins_operators, ins_fields, ins_bc, ins_adjoint, ins_temp_adjoint, ins_tensorclosure,
// ins_filter, ins_f32g): one work-item per volume, x along the 64-lane wavefront so every global access is a unit-stride row segment,
// 64x4 workgroups, any boundary conditions, 2-D (D = 2, k = 0) and 3-D.  Launch geometry, the index maps that undo it, the index-set
// masks and the by-dimension launch live here and nowhere else; the tuned kernels (flux, fast3d, FFT, register rows) keep their own.
#pragma once

#include "ins_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Launch geometry
// ------------------------------------------------------------------------------------------------
struct BoxMap {  // tiles of the banded order: ntx x nty tiles of 64x4 volumes per plane, nty_l = rows of tiles per XCD band
  int ntx, nty, nty_l;
};
struct Launch3 {
  dim3 grid, block;
  BoxMap map;  // banded launches only; the kernel takes it as its second argument
};

// Box [lo, hi) of the padded array as a 3-D grid: 64x4 tiles in x and y, one plane per grid layer.  Undone by INS_VOL_INDEX.
inline Launch3 box_launch(int D, const int* lo, const int* hi) {
  Launch3 l{};
  l.block = dim3(64, 4, 1);
  l.grid = dim3(cdiv(hi[0] - lo[0], 64), cdiv(hi[1] - lo[1], 4), (unsigned)(D == 3 ? hi[2] - lo[2] : 1));
  return l;
}
inline Launch3 box_launch(int D, const int* N) {  // the whole padded array
  const int lo[3] = {0, 0, 0};
  return box_launch(D, lo, N);
}

// ntx x nty tiles per layer, nz layers, as a 1-D grid of 64x4 workgroups with an XCD-aware order: workgroup ids are dealt round-robin to
// the 8 XCDs, so id & 7 selects one of 8 y-ranges and, inside it, tiles run x fastest, then y, then z.  Every XCD then walks ITS slab of
// rows plane after plane, and the k-1 / k+1 planes a stencil re-reads are still in that XCD's own 4 MB L2 (3 planes x 1/8 of the
// rows x 3 components = 0.6 MB at 256^3) instead of coming from HBM three times.
inline Launch3 banded_tiles(int ntx, int nty, int nz) {
  Launch3 l;
  l.block = dim3(64, 4, 1);
  l.map = BoxMap{ntx, nty, (nty + 7) / 8};
  l.grid = dim3(8u * ntx * l.map.nty_l * (unsigned)nz, 1, 1);
  return l;
}
// Box [lo, hi) in that order, one volume per work-item.  Undone by INS_BANDED_INDEX.
inline Launch3 banded_launch(int D, const int* lo, const int* hi) {
  return banded_tiles((int)cdiv(hi[0] - lo[0], 64), (int)cdiv(hi[1] - lo[1], 4), D == 3 ? hi[2] - lo[2] : 1);
}
inline Launch3 banded_launch(int D, const int* N) {
  const int lo[3] = {0, 0, 0};
  return banded_launch(D, lo, N);
}

// Boundary lines of direction be: one work-item per point of the full padded plane normal to be, ncomp planes.  Undone by INS_LINE_INDEX.
inline Launch3 line_launch(const GridDev& g, int be, int ncomp) {
  const int o0 = be == 0 ? 1 : 0, o1 = be == 2 ? 1 : 2;
  Launch3 l{};
  l.block = dim3(256, 1, 1);
  l.grid = dim3(cdiv(g.N[o0], 256), (unsigned)(g.D == 3 ? g.N[o1] : 1), (unsigned)ncomp);
  return l;
}

// Entries that do not take a z-slab of the multi-GPU decomposition (the Float32 family, the tensor-closure pullbacks) begin with this:
// INS_ERR_UNSUPPORTED and the error "<what>: <why>" if any side of the grid is a halo side.
inline int no_halo(const ins_grid* G, const char* what, const char* why = "slab (halo) grids run in fp64 only") {
  for (int a = 0; a < G->g.D; ++a)
    if (G->g.bc[a][0] == INS_BC_HALO || G->g.bc[a][1] == INS_BC_HALO) {
      ins_set_error("%s: %s", what, why);
      return INS_ERR_UNSUPPORTED;
    }
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------
// Index preambles.  Each declares i, j, k, I[3] and the linear index c = i + j sx[1] + k sx[2] inside a kernel template with `int D`.
// ------------------------------------------------------------------------------------------------
// box_launch: volume of the box starting at (l0, l1, l2); sx = the element strides of the array.  OUT, a condition on i, j, k, leaves the
// kernel: `i >= h0 || j >= h1` past the upper x / y faces of the box (ragged last tiles), `false` where the kernel's own mask does it.
#define INS_VOL_INDEX(sx, l0, l1, l2, OUT)             \
  const int i = (l0) + blockIdx.x * 64 + threadIdx.x;  \
  const int j = (l1) + blockIdx.y * 4 + threadIdx.y;   \
  const int k = D == 3 ? (l2) + (int)blockIdx.z : 0;   \
  if (OUT) return;                                     \
  const int I[3] = {i, j, k};                          \
  const long long c = i + j * (sx)[1] + k * (sx)[2];   \
  (void)I;                                             \
  (void)c

// banded_launch, with `GridDev g` and `BoxMap L` in scope: volume of the box [lo, hi)
#define INS_BANDED_INDEX(lo0, lo1, lo2, hi0, hi1)                            \
  int seq_ = (int)(blockIdx.x >> 3);                                         \
  const int tx_ = seq_ % L.ntx;                                              \
  seq_ /= L.ntx;                                                             \
  const int ty_ = (int)(blockIdx.x & 7) * L.nty_l + seq_ % L.nty_l;          \
  if (ty_ >= L.nty) return;                                                  \
  const int i = (lo0) + tx_ * 64 + threadIdx.x;                              \
  const int j = (lo1) + ty_ * 4 + threadIdx.y;                               \
  const int k = D == 3 ? (lo2) + seq_ / L.nty_l : 0;                         \
  if (i >= (hi0) || j >= (hi1)) return;                                      \
  const int I[3] = {i, j, k};                                                \
  const long long c = i + j * g.sx[1] + k * g.sx[2];                         \
  (void)I

// line_launch, with `GridDev g` in scope: (q0, q1) enumerate the two directions o0 (fastest) and o1 (3-D only) != be in memory order;
// base = offset of the line's volume 0
#define INS_LINE_INDEX(be)                         \
  const int o0 = (be) == 0 ? 1 : 0;                \
  const int o1 = (be) == 2 ? 1 : 2;                \
  const int q0 = blockIdx.x * 256 + threadIdx.x;   \
  const int q1 = D == 3 ? (int)blockIdx.y : 0;     \
  if (q0 >= g.N[o0]) return;                       \
  const long long base = q0 * g.sx[o0] + (D == 3 ? q1 * g.sx[o1] : 0)

// ------------------------------------------------------------------------------------------------
// Index-set masks.  Safe for any I, out-of-array indices included: grid creation (ins_grid.hip) enforces 1 <= ip_lo, ip_hi <= N - 1 and
// 1 <= iu_lo, iu_hi <= N - 1 (0 and 1 in the unused direction of a 2-D grid), so a true result implies 0 <= I < N.
// in_ip, in_iu and dof spell in_range's loop out on the fields of g: handing g.ip_lo / g.iu_lo[al] to in_range as pointers changed the
// register allocation of the pullback kernels (SGPR spills in k_convdiff_adjoint<3, 3, *>).
// ------------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ bool in_range(const int (&I)[3], const int* lo, const int* hi) {
  bool ok = true;
#pragma unroll
  for (int b = 0; b < D; ++b) ok = ok && (I[b] >= lo[b]) && (I[b] < hi[b]);
  return ok;
}

// Coordinates of I shifted by s in direction b: the three index arguments of the masks below.
#define INS_SH(I, b, s) ((I)[0] + ((b) == 0) * (s)), ((I)[1] + ((b) == 1) * (s)), ((I)[2] + ((b) == 2) * (s))

// I ∈ Ip: the pressure points
template <int D>
__device__ __forceinline__ bool in_ip(const GridDev& g, int i0, int i1, int i2) {
  const int I[3] = {i0, i1, i2};
  bool ok = true;
#pragma unroll
  for (int b = 0; b < D; ++b) ok = ok && I[b] >= g.ip_lo[b] && I[b] < g.ip_hi[b];
  return ok;
}

// I ∈ Iu[al]: the write set of gravity! and divoftensor!
template <int D>
__device__ __forceinline__ bool in_iu(const GridDev& g, int al, int i0, int i1, int i2) {
  const int I[3] = {i0, i1, i2};
  bool ok = true;
#pragma unroll
  for (int b = 0; b < D; ++b) ok = ok && I[b] >= g.iu_lo[al][b] && I[b] < g.iu_hi[al][b];
  return ok;
}

// I holds a degree of freedom of component al in the forward stencils (k_convdiff / k_pressuregradient): inside the 1..N-2 box in
// every direction and inside Iu[al].
template <int D>
__device__ __forceinline__ bool dof(const GridDev& g, int al, int i0, int i1, int i2) {
  const int I[3] = {i0, i1, i2};
  bool ok = true;
#pragma unroll
  for (int b = 0; b < D; ++b) ok = ok && I[b] >= 1 && I[b] <= g.N[b] - 2 && I[b] >= g.iu_lo[al][b] && I[b] < g.iu_hi[al][b];
  return ok;
}

// Transposed ghost copy of the BC pullbacks: x[from] = x[to] becomes (x̄[to] += x̄[from]; x̄[from] = 0).
template <typename T>
__device__ __forceinline__ void move_to(T* __restrict__ x, long long from, long long to) {
  const T t = x[from];
  x[from] = T(0);
  x[to] += t;
}

// ------------------------------------------------------------------------------------------------
// KERNEL names the instantiation with `D` for the dimension, e.g. (k_convdiff<D, MODE, OVERWRITE>): launched with D = 2 or 3 by the
// dimension of `g` (from the enclosing scope), then the launch check.  The arguments after the stream are the kernel's.
// ------------------------------------------------------------------------------------------------
#define INS_LAUNCH_D(KERNEL, launch, stream, ...)                                          \
  do {                                                                                     \
    const auto& launch_ = (launch);                                                        \
    if (g.D == 2) {                                                                        \
      constexpr int D = 2;                                                                 \
      hipLaunchKernelGGL(KERNEL, launch_.grid, launch_.block, 0, stream, __VA_ARGS__);     \
    } else {                                                                               \
      constexpr int D = 3;                                                                 \
      hipLaunchKernelGGL(KERNEL, launch_.grid, launch_.block, 0, stream, __VA_ARGS__);     \
    }                                                                                      \
    INS_LAUNCH_CHECK();                                                                    \
  } while (0)

}  // namespace
