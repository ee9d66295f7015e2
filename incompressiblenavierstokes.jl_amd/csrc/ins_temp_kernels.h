// Forward kernels of the temperature equation (operators.jl:59-62, 800-810, 914-931; boundary_conditions.jl:236-246, 338-513), once for
// both precisions: templates over the scalar type T of the fields, instantiated with double by ins_fields.hip and with float by
// ins_temp32.hip (two translation units, so that each keeps its register allocation).  One work-item per volume in the banded order of
// ins_stencil.h, 2-D and 3-D, periodic, Dirichlet, symmetric and pressure temperature sides, uniform and stretched grids.  The pullbacks of
// ins_temp_adjoint_kernels.h are the transposes of these.  k_convdiff_temp and k_temp_stage are NOT here: no spelling tried kept the code of
// both precisions (profiles/forward_generic_isa.md), so ins_fields.hip and ins_temp32.hip each keep theirs.
//
// The one rule for both precisions: the grid handle is the fp64 one, a metric table entry is read as a double and converted
// with (T) where it enters the arithmetic, constants are written T(…), and everything else is in T.  With T = double the conversions vanish.
#pragma once

#include "ins_stencil.h"

namespace {

// avg(ϕ, Δ, I, α)                                                               operators.jl:59-62
template <typename T>
__device__ __forceinline__ T avg_at(const GridDev& g, const T* __restrict__ phi, long long c, int ia, int a) {
  const T d0 = (T)g.dx[a][ia], d1 = (T)g.dx[a][ia + 1];
  return (d1 * phi[c] + d0 * phi[c + g.sx[a]]) / (d0 + d1);
}

// dissipation!: interpolation of u · diffusion(u) to the pressure points  (diss += ...)   operators.jl:800-810
template <int D, typename T>
__global__ __launch_bounds__(256) void k_dissipation_interp(GridDev g, BoxMap L, T coef, const T* __restrict__ u, const T* __restrict__ diff,
                                                            T* __restrict__ diss) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
  T d = T(0.0);
#pragma unroll
  for (int b = 0; b < D; ++b) {
    const T* ub = u + b * g.sc;
    const T* db = diff + b * g.sc;
    d += coef * (ub[c - g.sx[b]] * db[c - g.sx[b]] + ub[c] * db[c]) / 2;
  }
  diss[c] += d;
}

// gravity!  (F[:, gdir] += α2 avg(temp))   over the whole Iu[gdir]                     operators.jl:914-931
template <int D, typename T>
__global__ __launch_bounds__(256) void k_gravity(GridDev g, BoxMap L, int gdir, T a2, const T* __restrict__ temp, T* __restrict__ F) {
  INS_BANDED_INDEX(g.iu_lo[gdir][0], g.iu_lo[gdir][1], g.iu_lo[gdir][2], g.iu_hi[gdir][0], g.iu_hi[gdir][1]);
  F[gdir * g.sc + c] += a2 * avg_at<T>(g, temp, c, gdir == 0 ? i : (gdir == 1 ? j : k), gdir);
}

// apply_bc_temp!                               boundary_conditions.jl:236-246, 338-339, 391-405, 466-467, 512-513
// One work-item per point of the full padded plane (boundary(), :97-103).  Dirichlet value: constant, or a plane buffer (nullable).
template <typename T>
struct TempBC {
  int bc[2];
  T val[2];
  const T* plane[2];
};
template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_temp(GridDev g, T* __restrict__ temp, int be, TempBC<T> t) {
  INS_LINE_INDEX(be);
  const long long sb = g.sx[be];
  const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
  if (t.bc[0] == INS_BC_PERIODIC) {
    temp[base + ia * sb] = temp[base + (ib - 1) * sb];
    temp[base + ib * sb] = temp[base + (ia + 1) * sb];
    return;
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int bc = t.bc[side];
    const int i = side ? ib : ia;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_DIRICHLET)
      temp[base + i * sb] = t.plane[side] ? t.plane[side][q0 + (long long)q1 * g.N[o0]] : t.val[side];
    else if (bc == INS_BC_SYMMETRIC || bc == INS_BC_PRESSURE)
      temp[base + i * sb] = temp[base + jn * sb];
  }
}

}  // namespace
