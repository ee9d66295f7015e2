// Observer kernels of the processors (operators.jl:985-1020, 1311-1370, 1440-1460: vorticity!, interpolate_u_p!, interpolate_ω_p!, Qfield!), once
// for both precisions: templates over the scalar type T of the fields, instantiated with double by ins_fields.hip and with float by
// ins_fields32.hip (two translation units, so that each keeps its register allocation).  One work-item per volume in the banded order of
// ins_stencil.h, 2-D and 3-D, any boundary conditions, uniform and stretched grids.  The fp64 device code of the four kernels is what it was
// when they were written in double inside ins_fields.hip (profiles/fields32_generic_isa.md).
//
// The one rule for both precisions: the grid handle is the fp64 one, a metric table entry is read as a double and converted
// with (T) where it enters the arithmetic, constants are written T(…), and everything else is in T.  With T = double the conversions vanish.
#pragma once

#include "ins_stencil.h"

namespace {

// --------------------------------------------------------------------------------------------
// vorticity!                                             operators.jl:985-1020 (ndrange = N .- 1)
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_vorticity(GridDev g, BoxMap L, const T* __restrict__ u, T* __restrict__ w) {
  INS_BANDED_INDEX(0, 0, 0, g.N[0] - 1, g.N[1] - 1);
  if (D == 2) {
    const T* u0 = u;
    const T* u1 = u + g.sc;
    w[c] = (u1[c + g.sx[0]] - u1[c]) * (T)g.rdxu[0][i] - (u0[c + g.sx[1]] - u0[c]) * (T)g.rdxu[1][j];
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int ap = (a + 1) % 3, am = (a + 2) % 3;
      const T* up = u + ap * g.sc;
      const T* um = u + am * g.sc;
      w[a * g.sc + c] = (um[c + g.sx[ap]] - um[c]) * (T)g.rdxu[ap][I[ap]] - (up[c + g.sx[am]] - up[c]) * (T)g.rdxu[am][I[am]];
    }
  }
}

// interpolate_u_p!                                                     operators.jl:1311-1326
template <int D, typename T>
__global__ __launch_bounds__(256) void k_interp_u_p(GridDev g, BoxMap L, const T* __restrict__ u, T* __restrict__ up) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* ua = u + a * g.sc;
    up[a * g.sc + c] = (ua[c - g.sx[a]] + ua[c]) / 2;
  }
}

// interpolate_ω_p!                                                     operators.jl:1336-1370
template <int D, typename T>
__global__ __launch_bounds__(256) void k_interp_w_p(GridDev g, BoxMap L, const T* __restrict__ w, T* __restrict__ wp) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
  if (D == 2) {
    wp[c] = (w[c - g.sx[0] - g.sx[1]] + w[c]) / 2;
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int ap = (a + 1) % 3, am = (a + 2) % 3;
      const T* wa = w + a * g.sc;
      wp[a * g.sc + c] = (wa[c - g.sx[ap] - g.sx[am]] + wa[c]) / 2;
    }
  }
}

// Qfield!                                                              operators.jl:1440-1460
template <int D, typename T>
__global__ __launch_bounds__(256) void k_Qfield(GridDev g, BoxMap L, const T* __restrict__ u, T* __restrict__ Q) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
  T q = T(0.0);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* ua = u + a * g.sc;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const T* ub = u + b * g.sc;
      q -= (ua[c] - ua[c - g.sx[b]]) * (T)g.rdx[b][I[b]] * (ub[c] - ub[c - g.sx[a]]) * (T)g.rdx[a][I[a]] / 2;
    }
  }
  Q[c] = q;
}

}  // namespace
