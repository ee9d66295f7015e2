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

// β_i of the stage-velocity basis (beta[0..i-1]): back-substitution, A lower triangular
static inline void ins_rk_beta(const double* A, int ns, int i, double* beta) {
  const double* row = A + i * ns;
  for (int m = i - 1; m >= 0; --m) {
    double v = row[m];
    for (int j = m + 1; j < i; ++j) v -= beta[j] * A[j * ns + m];
    beta[m] = v / A[m * ns + m];
  }
}

enum RkBasis { RK_K_BASIS, RK_V_BASIS };
// The steady body force f (k_j = F_j + f, operators.jl:873-880; the arrays hold F_j only) enters with Δt Σ_{j<=i} A[i,j] in the k-basis and with
// Δt A[i,i] in the stage-velocity basis (the V_m already hold their share).  The k-basis sum is formed in one of two orders, one ulp apart:
//   RK_FORCE_DIAG_FIRST   Δt A[i,i] + Δt A[i,0] + .. + Δt A[i,i-1]   3-D periodic, tiled and ext fused periodic loops (rk_step_fused_periodic,
//                                                                    rk_step_any, ins_rk_step_ext_f64's first branch)
//   RK_FORCE_INDEX_ORDER  0 + Δt A[i,0] + .. + Δt A[i,i]             2-D periodic and ext tiled loops (rk_step_fused_periodic_2d, ins_rk_step_ext_f64's
//                                                                    second branch) and the reference-order lists (ins_rk_sum_terms)
enum RkForceOrder { RK_FORCE_DIAG_FIRST, RK_FORCE_INDEX_ORDER };

// A zeroed RkEpi with n, coef[], k[], c0m1, self_in, coef_self and write_k of stage i filled.  prev[m]: the array of earlier stage m (k_m or V_m; any table of pointers or of buffers; P =
// float on the Float32 path, whose kernels cast RkEpi's untyped pointers back); force: nullptr or the steady body force, always the last term.
// input_in_regs (stage-velocity basis): V_{i-1} is the stencil input and the kernel keeps its uncorrected value in registers, so β_{i,i-1} goes to
// self_in instead of a term that would be loaded.  Terms with a zero coefficient are skipped.
template <typename P, typename Prev>
static inline RkEpi ins_rk_stage_terms(const double* A, int ns, int i, double dt, const Prev& prev, const P* force, RkBasis basis, bool input_in_regs,
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
    ins_rk_beta(A, ns, i, beta);
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

// Carrying a combination forward (stage-velocity basis, the stencil input in registers).  The last stage i of RK44 loads ustart, V_0 and V_1 only to form
//   -1/3 ustart + 1/3 V_0 + 2/3 V_1        (β_3 = (1/3, 2/3, 1/3); V_2 is its stencil input),
// and stage j = 1 has all three in registers: ustart is its combination s before Δt A[j,j] f is added (its own β_j is zero, so s = 1·ustart), V_0 its
// stencil input (the uncorrected copy the correcting kernel keeps) and V_1 what it stores.  So stage j also stores S = a0 s + a1 V_{j-1} + a2 V_j (24 B per
// cell written) and stage i starts from S instead of loading three arrays (48 B per cell not read).
// A plan exists when
//   * i = ns - 1 and j = i - 2 >= 1: one stage lies between them, and it gives its output buffer to S and stores V_{j+1} where V_{j-1} was;
//   * of stage i's loaded terms (β_i[m], m < i - 1) only m = j - 1 and m = j are non-zero, β_i[j] among them, and c0 = 1 - Σ β_i is non-zero;
//   * β_j = 0, so that stage j's s is ustart exactly (plus the body force's share, below);
//   * stage j + 1 does not load V_{j-1} (β_{j+1}[j-1] = 0): nothing between j and i needs what the plan displaces.
// Every other tableau (Wray3, SSP33, FE11, ...) has no plan (j = -1) and runs as without this.
// With a steady body force stage j's s is ustart + Δt A[j,j] f, so S holds a0 Δt A[j,j] f too much: stage i's own force coefficient gives it back.
struct RkCarryPlan {
  int j, i;     // producing and consuming stage; j < 0: no plan
  double a[3];  // S = a[0] ustart + a[1] V_{j-1} + a[2] V_j: the c0 and β of ins_rk_stage_terms, bit for bit
};
static inline RkCarryPlan ins_rk_carry_plan(const double* A, int ns) {
  RkCarryPlan pl = {-1, -1, {0.0, 0.0, 0.0}};
  const int i = ns - 1, j = ns - 3;
  if (j < 1 || !ins_rk_vbasis_possible(A, ns)) return pl;
  double bi[INS_MAX_STAGES], bj[INS_MAX_STAGES], bn[INS_MAX_STAGES];
  ins_rk_beta(A, ns, i, bi);
  ins_rk_beta(A, ns, j, bj);
  ins_rk_beta(A, ns, j + 1, bn);
  for (int m = 0; m < j; ++m)
    if (bj[m] != 0.0) return pl;
  for (int m = 0; m < j - 1; ++m)
    if (bi[m] != 0.0) return pl;
  if (bi[j] == 0.0 || bn[j - 1] != 0.0) return pl;
  double c0m1 = 0.0;  // the order of ins_rk_stage_terms
  for (int m = 0; m < i; ++m)
    if (bi[m] != 0.0) c0m1 -= bi[m];
  if (1.0 + c0m1 == 0.0) return pl;
  pl.j = j;
  pl.i = i;
  pl.a[0] = 1.0 + c0m1;
  pl.a[1] = bi[j - 1];
  pl.a[2] = bi[j];
  return pl;
}

// Stage pl.i with the plan: it starts from S (RkEpi::ustart = S, factor 1), adds β_{i,i-1} times its stencil input from registers and, last, the body force.
template <typename P>
static inline RkEpi ins_rk_carry_consumer_terms(const double* A, int ns, const RkCarryPlan& pl, double dt, const P* S, const P* force) {
  RkEpi epi;
  memset(&epi, 0, sizeof(epi));
  const int i = pl.i;
  double beta[INS_MAX_STAGES];
  ins_rk_beta(A, ns, i, beta);
  epi.ustart = reinterpret_cast<const double*>(S);
  epi.self_in = beta[i - 1];
  if (force) {
    epi.coef[0] = dt * A[i * ns + i] - pl.a[0] * (dt * A[pl.j * ns + pl.j]);
    epi.k[0] = reinterpret_cast<const double*>(force);
    epi.n = 1;
  }
  epi.coef_self = dt * A[i * ns + i];
  return epi;
}

// The reference-order list u = ustart + Σ_{j<=i} Δt A[i,j] k_j of the loops that run the reference's kernel sequence (the combine kernels): writes the
// non-zero coefficients and their arrays to coef[] / k[] (room for INS_MAX_STAGES + 1), then the body force with Σ_{j<=i} Δt A[i,j] in index order
// (zeros included: they add nothing), and returns the number of terms.  The products are formed in S, the caller's precision: the Float32 loop
// multiplies Δt (float)A[i,j] in float.
template <typename S, typename P, typename Prev>
static inline int ins_rk_sum_terms(const double* A, int ns, int i, S dt, const Prev& prev, const P* force, S* coef, const P** k) {
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
