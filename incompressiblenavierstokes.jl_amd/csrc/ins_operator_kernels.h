// The divergence and the ghost fills of velocity and pressure (operators.jl:81-125; boundary_conditions.jl:159-502), once for both
// precisions: templates over the scalar type T of the fields, instantiated with double by ins_operators.hip / ins_bc.hip and with float by
// ins_f32g.hip (separate translation units, so that each keeps its register allocation).  One work-item per volume, x along the 64-lane
// wavefront, 2-D and 3-D, any BC mix, uniform and stretched grids.  The pullbacks of ins_adjoint_kernels.h are the transposes of these.
// k_convdiff and k_pressuregradient are NOT here: their float copies fuse other multiply-adds (see k32g_momentum in ins_f32g.hip).
//
// The one rule for both precisions: the grid handle is the fp64 one, a metric table entry is read as a double and converted
// with (T) where it enters the arithmetic, constants are written T(…), and everything else is in T.  With T = double the conversions vanish.
#pragma once

#include "ins_stencil.h"

namespace {

// divergence! on Ip (operators.jl:117-125) of a field of type T into an array of type P, the differences taken in P.  SCALE: times the
// volume (scalewithvolume!, operators.jl:81-95).  <float, double, true> forms the right-hand side of the fp64 solver a Float32 solver wraps.
template <int D, typename T, typename P, bool SCALE>
__global__ __launch_bounds__(256) void k_divergence(GridDev g, const T* __restrict__ u, P* __restrict__ div) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], i >= g.ip_hi[0] || j >= g.ip_hi[1]);
  P d = P(0.0);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* ua = u + a * g.sc;
    d += ((P)ua[c] - (P)ua[c - g.sx[a]]) * (P)g.rdx[a][I[a]];
  }
  if (SCALE) {
    P om = (P)g.dx[0][i] * (P)g.dx[1][j];
    if (D == 3) om *= (P)g.dx[2][k];
    d *= om;
  }
  div[c] = d;
}

// apply_bc_u!                                   boundary_conditions.jl:159-206, 276-288, 344-375, 414-428, 472-482
// One launch per direction β (the reference sweeps β = 1..D in order so that edges and corners come out right, :162-165); work-items span
// the full padded extent of the other directions (`boundary()`, :97-103) times the D components.  Plane coordinates (q0, q1) enumerate
// the two directions != β in memory order.  Dirichlet value: a plane buffer (planes nullable, and each of its entries), zero (dudt) or the
// constant of the grid.  A HALO side is filled by the caller (slab neighbour exchange).
template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_u(GridDev g, T* __restrict__ u, int be, int dudt, const T* const* planes) {
  INS_LINE_INDEX(be);
  const int al = blockIdx.z;
  const long long sb = g.sx[be];
  T* ua = u + al * g.sc;
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  if (bcl == INS_BC_PERIODIC) {  // both sides in one go
    const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
    ua[base + ia * sb] = ua[base + (ib - 1) * sb];
    ua[base + ib * sb] = ua[base + (ia + 1) * sb];
    return;
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int bc = side ? bcr : bcl;
    if (bc == INS_BC_HALO) continue;
    const int i = side ? g.iu_hi[al][be] : g.iu_lo[al][be] - 1;
    const int jn = side ? i - 1 : i + 1;
    T* dst = ua + base + i * sb;
    if (bc == INS_BC_DIRICHLET) {
      const T* pl = planes ? planes[(be * 2 + side) * 3 + al] : nullptr;
      T v;
      if (pl)
        v = pl[q0 + (D == 3 ? (long long)q1 * g.N[o0] : 0)];
      else
        v = dudt ? T(0.0) : (T)g.bc_u[be][side][al];
      *dst = v;
    } else if (bc == INS_BC_SYMMETRIC) {
      *dst = (al == be) ? T(0.0) : ua[base + jn * sb];
    } else if (bc == INS_BC_PRESSURE) {
      *dst = ua[base + jn * sb];
    }
  }
}

// apply_bc_p!                                   boundary_conditions.jl:306-318, 388, 445-453, 497-502
// blockIdx.z selects one of several scalar fields fstride elements apart.  Dirichlet: no-op (:388); HALO: caller.
template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_p(GridDev g, T* __restrict__ p, int be, long long fstride) {
  p += (long long)blockIdx.z * fstride;
  INS_LINE_INDEX(be);
  const long long sb = g.sx[be];
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
  if (bcl == INS_BC_PERIODIC) {
    p[base + ia * sb] = p[base + (ib - 1) * sb];
    p[base + ib * sb] = p[base + (ia + 1) * sb];
    return;
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int bc = side ? bcr : bcl;
    const int i = side ? ib : ia;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_SYMMETRIC)
      p[base + i * sb] = p[base + jn * sb];
    else if (bc == INS_BC_PRESSURE)
      p[base + i * sb] = T(0.0);
  }
}

}  // namespace
