// The tableau-dependent part of a Runge-Kutta stage, built on the host: which earlier-stage arrays stage i of the shifted tableau A (ns x ns, lower
// triangular, row i = the weights of u_{i+1}) combines and with which coefficients.  Plain C++, no HIP call; every stage loop (ins_rk.hip,
// ins_rk_ext.hip, ins_f32.hip) gets its terms here and adds only its own pointers (ustart / ustar, the closure and temperature fields, rhs_out).
//
// Two bases.
//   k-basis               u* = ustart + Σ_{j<i} Δt A[i,j] k_j + Δt A[i,i] k_i                      (step_explicit_runge_kutta.jl:35-38, same order)
//   stage-velocity basis  with the in-kernel correction the UNCORRECTED stage velocities V_m = ustart + Δt Σ_{j<=m} A[m,j] k_j stay in memory anyway
//     (they are the next stencil's input), and when every A[m,m] != 0 they span the same space as {ustart, k_j}:
//         V_i = (1 - Σ_m β_im) ustart + Σ_{m<i} β_im V_m + Δt A[i,i] k_i,     β_i · A[0:i,0:i] = A[i,0:i].
//     So no k_j is ever written or read: RK44 moves 336 instead of 432 B per cell and step through the periodic stage kernels (360 on the tiled path,
//     which reads V_{i-1} from memory), with β_3 = (1/3, 2/3, 1/3) and every other β = 0.  Algebraically the reference's combination; rounding differs
//     at the 1e-16 level.  INS_RK_KEEP_K=1 restores the k-basis at every call site.
#pragma once

#include "ins_internal.h"

// the stage-velocity basis exists: every V_m contains its own k_m
static inline bool ins_rk_vbasis_possible(const double* A, int ns) {
  for (int m = 0; m < ns; ++m)
    if (A[m * ns + m] == 0.0) return false;
  return true;
}

// a later row of the tableau reads k_i: the stage has to store it (k-basis)
static inline bool ins_rk_needed_later(const double* A, int ns, int i) {
  for (int i2 = i + 1; i2 < ns; ++i2)
    if (A[i2 * ns + i] != 0.0) return true;
  return false;
}

enum RkBasis { RK_K_BASIS, RK_V_BASIS };
// The steady body force f (k_j = F_j + f, operators.jl:873-880; the arrays hold F_j only) enters with Δt Σ_{j<=i} A[i,j] in the k-basis and with
// Δt A[i,i] in the stage-velocity basis (the V_m already hold their share).  The k-basis sum is formed in one of two orders, one ulp apart:
//   RK_FORCE_DIAG_FIRST   Δt A[i,i] + Δt A[i,0] + .. + Δt A[i,i-1]   3-D periodic, tiled and ext fused periodic loops (rk_step_fused_periodic,
//                                                                    rk_step_any, ins_rk_step_ext_f64's first branch)
//   RK_FORCE_INDEX_ORDER  0 + Δt A[i,0] + .. + Δt A[i,i]             2-D periodic and ext tiled loops (rk_step_fused_periodic_2d, ins_rk_step_ext_f64's
//                                                                    second branch) and the reference-order lists (ins_rk_sum_terms)
enum RkForceOrder { RK_FORCE_DIAG_FIRST, RK_FORCE_INDEX_ORDER };

// A zeroed RkEpi with n, coef[], k[], c0m1, self_in, coef_self and write_k of stage i filled.  prev[m]: the array of earlier stage m (k_m or V_m; P =
// float on the Float32 path, whose kernels cast RkEpi's untyped pointers back); force: nullptr or the steady body force, always the last term.
// input_in_regs (stage-velocity basis): V_{i-1} is the stencil input and the kernel keeps its uncorrected value in registers, so β_{i,i-1} goes to
// self_in instead of a term that would be loaded.  Terms with a zero coefficient are skipped.
template <typename P>
static inline RkEpi ins_rk_stage_terms(const double* A, int ns, int i, double dt, P* const* prev, const P* force, RkBasis basis, bool input_in_regs,
                                       RkForceOrder order) {
  RkEpi epi;
  memset(&epi, 0, sizeof(epi));
  const double* row = A + i * ns;
  auto term = [&](double coef, const P* k) {
    epi.coef[epi.n] = coef;
    epi.k[epi.n] = reinterpret_cast<const double*>(k);
    ++epi.n;
  };
  if (basis == RK_V_BASIS) {
    double beta[INS_MAX_STAGES];
    for (int m = i - 1; m >= 0; --m) {  // back-substitution, A lower triangular
      double v = row[m];
      for (int j = m + 1; j < i; ++j) v -= beta[j] * A[j * ns + m];
      beta[m] = v / A[m * ns + m];
    }
    for (int m = 0; m < i; ++m) {
      if (beta[m] == 0.0) continue;
      epi.c0m1 -= beta[m];
      if (m == i - 1 && input_in_regs)
        epi.self_in = beta[m];
      else
        term(beta[m], prev[m]);
    }
  } else {
    for (int j = 0; j < i; ++j) {
      const double coef = dt * row[j];
      if (coef != 0.0) term(coef, prev[j]);
    }
    epi.write_k = ins_rk_needed_later(A, ns, i);
  }
  if (force) {
    double cf = order == RK_FORCE_DIAG_FIRST ? dt * row[i] : 0.0;
    if (basis == RK_K_BASIS)
      for (int j = 0; j < i; ++j) cf += dt * row[j];
    if (order == RK_FORCE_INDEX_ORDER) cf += dt * row[i];
    term(cf, force);
  }
  epi.coef_self = dt * row[i];
  return epi;
}

// The reference-order list u = ustart + Σ_{j<=i} Δt A[i,j] k_j of the loops that run the reference's kernel sequence (the combine kernels): writes the
// non-zero coefficients and their arrays to coef[] / k[] (room for INS_MAX_STAGES + 1), then the body force with Σ_{j<=i} Δt A[i,j] in index order
// (zeros included: they add nothing), and returns the number of terms.  The products are formed in S, the caller's precision: the Float32 loop
// multiplies Δt (float)A[i,j] in float.
template <typename S, typename P>
static inline int ins_rk_sum_terms(const double* A, int ns, int i, S dt, P* const* prev, const P* force, S* coef, const P** k) {
  int n = 0;
  S cf = 0;
  for (int j = 0; j <= i; ++j) {
    const S c = dt * (S)A[i * ns + j];
    cf += c;
    if (c == 0) continue;
    coef[n] = c;
    k[n] = prev[j];
    ++n;
  }
  if (force) {
    coef[n] = cf;
    k[n] = force;
    ++n;
  }
  return n;
}
