// The reverse stage loop of one explicit Runge-Kutta step, written once for T ∈ {double, float} and for the state u or (u, temp): what
// ins_rk_step_pullback_f32 and ins_rk_step_pullback_ext_f64 / _f32 run (csrc/ins_rk_adjoint.hip).  The transpose of the loop of
// `_autodiff_core.timestep` (step_explicit_runge_kutta.jl:61-120).
//
// Forward, stage i = 0..s-1, u_0 = ustart, T_0 = tempstart (A the shifted tableau, f the steady body force or 0):
//     v_i = bc_u(u_i)   τ_i = bc_T(T_i)
//     k_i = F(v_i) + gravity(τ_i) + f [+ m(v_i, θ)]         c_i = convdiff_temp(v_i, τ_i) + [diss] dissipation(v_i)
//     w_i = ustart + Δt Σ_j A[i,j] k_j                      T_{i+1} = tempstart + Δt Σ_j A[i,j] c_j
//     u_{i+1} = P(bc_u(w_i));                               u_out = bc_u(u_s), temp_out = bc_T(T_s)
// Reverse, (g_u, g_T) the cotangents of (v_{i+1}, τ_{i+1}), of (u_out, temp_out) at the start:
//     ȳ_i = bc_uᵀ Pᵀ bc_uᵀ g_u                              z̄_i = bc_Tᵀ g_T
//     k̄_i = Δt Σ_{i'>=i} A[i',i] ȳ_{i'}                     c̄_i = Δt Σ_{i'>=i} A[i',i] z̄_{i'}
//     g_u = J_F(v_i)ᵀ k̄_i, then the temperature stage pullback at (v_i, τ_i) with (Fbar, cbar) = (k̄_i, c̄_i): g_u +=, g_T =
// and ∂L/∂ustart = Σ_i ȳ_i + bc_uᵀ g_u, ∂L/∂tempstart = Σ_i z̄_i + bc_Tᵀ g_T.
// With the Smagorinsky closure m (set_closure; the order of `_autodiff_core.timestep`: momentum (+ gravity), body force, closure) the recomputation adds
// ins_smagorinsky_force_* at v_i as one more term of the combination, and the reverse sweep adds its pullback at (v_i, k̄_i) after the momentum
// pullback:  g_u += (∂m/∂u)ᵀ k̄_i,  *thetabar += (∂m/∂θ)ᵀ k̄_i  (ins_smagorinsky_force_pullback_*).
//
// The (v_i, τ_i) are recomputed with the operator-level entries of the respective family, as the isothermal fp64 loop does.  k̄_i and c̄_i are
// formed by ONE launch (k_adj_stage_sums) and the two closing sums by one more (k_adj_close_sums): streaming kernels, 16-byte accesses where
// every array is 16-byte aligned, terms in index order, zero coefficients skipped.  The combination is never fused into the pullback kernels
// here (INS_ADJ_STAGE_FUSED is the fp64 isothermal loop's): the two-launch form is the measured-faster one.
#pragma once
#include "ins_f32_internal.h"
#include "ins_internal.h"
#include "ins_rk_terms.h"

#include <cstdint>

// Work arrays of the reverse step.  v, y: nstage vector fields each; kbar: one; pwork: one scalar.  With a temperature: tau, z (nstage scalars each)
// and cbar, allocated by set_temperature.
template <typename T, typename PS>
struct RkAdjointT {
  const ins_grid* grid = nullptr;  // borrowed
  PS* ps = nullptr;                // borrowed
  int nstage = 0;
  std::vector<double> A, c;
  std::vector<DevBuf<T>> v;  // stage inputs v_i (ghosts filled)
  std::vector<DevBuf<T>> y;  // k_i during the recomputation, then the stage cotangents ȳ_i
  DevBuf<T> kbar;     // k̄_i; the `diff` scratch of dissipation! during the recomputation
  DevBuf<T> pwork;
  bool temp_on = false;
  ins_temperature_desc_t td{};
  std::vector<DevBuf<T>> tau;  // stage temperatures τ_i (ghosts filled)
  std::vector<DevBuf<T>> z;    // c_i during the recomputation, then the stage cotangents z̄_i
  DevBuf<T> cbar;
  // Smagorinsky closure (set_closure): θ, the device double that collects ∂L/∂θ (nullable), the closure force of the stage being recomputed and the
  // `sigma` scratch of the three-kernel force (where ins_smagorinsky_force_needs_sigma answers 1)
  int closure_kind = 0;
  double theta = 0.0;
  double* thetabar = nullptr;  // borrowed
  DevBuf<T> mforce;
  DevBuf<T> sigma;
};

namespace rkadj {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T>
struct Vec16;
template <>
struct Vec16<double> {
  using type = f64x2;
  static constexpr int L = 2;
};
template <>
struct Vec16<float> {
  using type = f32x4;
  static constexpr int L = 4;
};

// the non-zero terms of one reverse stage: weights, the vector fields ȳ_{i'} and (nc > 0) the scalar fields z̄_{i'}
template <typename T>
struct Terms {
  int n;
  T w[INS_MAX_STAGES];
  const T* y[INS_MAX_STAGES];
  const T* z[INS_MAX_STAGES];
};

// out[t] = (CLOSE ? out[t] + Σ_q p[q][t] : Σ_q w[q]·p[q][t]), t < n, terms in index order.  VEC: every array is 16-byte aligned; n / L vectors,
// then the n % L elements left.
template <typename T, bool VEC, bool CLOSE>
__device__ __forceinline__ void sum_range(long long n, T* out, const T* const* p, const T* w, int nt) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  long long done = 0;
  if constexpr (VEC) {
    using V = typename Vec16<T>::type;
    constexpr int L = Vec16<T>::L;
    const long long nvec = n / L;
    V* outv = reinterpret_cast<V*>(out);
    for (long long t = tid; t < nvec; t += stride) {
      V a = CLOSE ? outv[t] : V(0);
      for (int q = 0; q < nt; ++q) {
        const V x = reinterpret_cast<const V*>(p[q])[t];
        if constexpr (CLOSE)
          a += x;
        else
          a += w[q] * x;
      }
      outv[t] = a;
    }
    done = nvec * L;
  }
  for (long long t = done + tid; t < n; t += stride) {
    T a = CLOSE ? out[t] : T(0);
    for (int q = 0; q < nt; ++q) {
      if constexpr (CLOSE)
        a += p[q][t];
      else
        a += w[q] * p[q][t];
    }
    out[t] = a;
  }
}

// k̄_i = Σ_q w[q]·ȳ_q over a vector field (nv elements) and c̄_i = Σ_q w[q]·z̄_q over a scalar field (nc elements; 0: isothermal), one launch
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_adj_stage_sums(long long nv, long long nc, T* __restrict__ kbar, T* __restrict__ cbar, Terms<T> ts) {
  sum_range<T, VEC, false>(nv, kbar, ts.y, ts.w, ts.n);
  if (nc) sum_range<T, VEC, false>(nc, cbar, ts.z, ts.w, ts.n);
}

// ubar += Σ_i ȳ_i and tempbar += Σ_i z̄_i (nc = 0: isothermal), in place, one launch
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_adj_close_sums(long long nv, long long nc, T* __restrict__ ubar, T* __restrict__ tempbar, Terms<T> ts) {
  sum_range<T, VEC, true>(nv, ubar, ts.y, ts.w, ts.n);
  if (nc) sum_range<T, VEC, true>(nc, tempbar, ts.z, ts.w, ts.n);
}

template <typename T>
inline bool aligned16(const T* outv, const T* outc, const Terms<T>& ts, bool with_temp) {
  uintptr_t bits = reinterpret_cast<uintptr_t>(outv) | (with_temp ? reinterpret_cast<uintptr_t>(outc) : 0);
  for (int q = 0; q < ts.n; ++q) bits |= reinterpret_cast<uintptr_t>(ts.y[q]) | (with_temp ? reinterpret_cast<uintptr_t>(ts.z[q]) : 0);
  return (bits & 15) == 0;
}

template <typename T, bool CLOSE>
inline int launch_sums(long long nv, long long nc, T* outv, T* outc, const Terms<T>& ts, hipStream_t s) {
  const bool vec = aligned16(outv, outc, ts, nc > 0);
  const long long work = vec ? (nv + Vec16<T>::L - 1) / Vec16<T>::L : nv;  // the vector field sets the grid; the scalar field strides over it
  const unsigned nblk = (unsigned)std::max<long long>(1, std::min<long long>((work + 255) / 256, 8192));
  if (vec) {
    if (CLOSE)
      hipLaunchKernelGGL((k_adj_close_sums<T, true>), dim3(nblk), dim3(256), 0, s, nv, nc, outv, outc, ts);
    else
      hipLaunchKernelGGL((k_adj_stage_sums<T, true>), dim3(nblk), dim3(256), 0, s, nv, nc, outv, outc, ts);
  } else {
    if (CLOSE)
      hipLaunchKernelGGL((k_adj_close_sums<T, false>), dim3(nblk), dim3(256), 0, s, nv, nc, outv, outc, ts);
    else
      hipLaunchKernelGGL((k_adj_stage_sums<T, false>), dim3(nblk), dim3(256), 0, s, nv, nc, outv, outc, ts);
  }
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// ---- the operator-level entries of the two families under one spelling
inline int bc_u(const ins_grid* G, double* u, hipStream_t s) { return ins_k_apply_bc_u(G, u, 0, nullptr, s); }
inline int bc_u(const ins_grid* G, float* u, hipStream_t s) { return ins_apply_bc_u_f32(G, u, s); }
inline int bc_temp(const ins_grid* G, const ins_temperature_desc_t& td, double* t, hipStream_t s) {
  return ins_apply_bc_temp_f64(G, td.bc, td.val, nullptr, t, s);
}
inline int bc_temp(const ins_grid* G, const ins_temperature_desc_t& td, float* t, hipStream_t s) {
  float val[6];
  for (int q = 0; q < 6; ++q) val[q] = (float)td.val[q];
  return ins_apply_bc_temp_f32(G, td.bc, val, t, s);
}
inline int momentum(const ins_grid* G, double visc, const double* u, double* F, hipStream_t s) { return ins_k_momentum(G, visc, u, F, s); }
inline int momentum(const ins_grid* G, float visc, const float* u, float* F, hipStream_t s) { return ins_momentum_f32(G, visc, u, F, s); }
inline int gravity(const ins_grid* G, const ins_temperature_desc_t& td, const double* t, double* F, hipStream_t s) {
  return ins_gravity_f64(G, td.gdir, td.a2, t, F, s);
}
inline int gravity(const ins_grid* G, const ins_temperature_desc_t& td, const float* t, float* F, hipStream_t s) {
  return ins_gravity_f32(G, td.gdir, (float)td.a2, t, F, s);
}
inline int convdiff_temp(const ins_grid* G, const ins_temperature_desc_t& td, const double* u, const double* t, double* c, hipStream_t s) {
  return ins_convection_diffusion_temp_f64(G, td.a4, u, t, c, s);
}
inline int convdiff_temp(const ins_grid* G, const ins_temperature_desc_t& td, const float* u, const float* t, float* c, hipStream_t s) {
  return ins_convection_diffusion_temp_f32(G, (float)td.a4, u, t, c, s);
}
inline int dissipation(const ins_grid* G, const ins_temperature_desc_t& td, double visc, const double* u, double* diff, double* c, hipStream_t s) {
  return ins_dissipation_f64(G, visc, td.diss_coef, u, diff, c, s);
}
inline int dissipation(const ins_grid* G, const ins_temperature_desc_t& td, float visc, const float* u, float* diff, float* c, hipStream_t s) {
  return ins_dissipation_f32(G, visc, (float)td.diss_coef, u, diff, c, s);
}
inline int combine(const ins_grid* G, long long n, const double* base, double* out, int nt, const double* coef, const double* const* k, hipStream_t s) {
  return n == G->ncell ? ins_combine_scalar_f64(G, base, out, nt, coef, k, s) : ins_combine_f64(G, base, out, nt, coef, k, s);
}
inline int combine(const ins_grid*, long long n, const float* base, float* out, int nt, const float* coef, const float* const* k, hipStream_t s) {
  return ins_k32_combine(n, base, out, nt, coef, k, s);
}
inline int project(const ins_grid* G, ins_poisson* ps, double* u, double* p, hipStream_t s) { return ins_k_project(G, ps, u, p, s); }
inline int project(const ins_grid* G, ins_poisson32* ps, float* u, float* p, hipStream_t s) { return ins_project_f32(G, ps, u, p, s); }
inline int bc_u_pullback(const ins_grid* G, double* g, hipStream_t s) { return ins_k_apply_bc_u_pullback(G, g, s); }
inline int bc_u_pullback(const ins_grid* G, float* g, hipStream_t s) { return ins_apply_bc_u_pullback_f32(G, g, s); }
inline int bc_temp_pullback(const ins_grid* G, const ins_temperature_desc_t& td, double* g, hipStream_t s) {
  return ins_apply_bc_temp_pullback_f64(G, td.bc, g, s);
}
inline int bc_temp_pullback(const ins_grid* G, const ins_temperature_desc_t& td, float* g, hipStream_t s) {
  return ins_apply_bc_temp_pullback_f32(G, td.bc, g, s);
}
inline int project_pullback(const ins_grid* G, ins_poisson* ps, double* g, double* p, hipStream_t s) { return ins_project_pullback_f64(G, ps, g, p, s); }
inline int project_pullback(const ins_grid* G, ins_poisson32* ps, float* g, float* p, hipStream_t s) { return ins_project_pullback_f32(G, ps, g, p, s); }
inline int momentum_pullback(const ins_grid* G, double visc, const double* u, const double* phibar, double* ubar, hipStream_t s) {
  return ins_momentum_pullback_f64(G, visc, u, phibar, ubar, 0, s);
}
inline int momentum_pullback(const ins_grid* G, float visc, const float* u, const float* phibar, float* ubar, hipStream_t s) {
  return ins_momentum_pullback_f32(G, visc, u, phibar, ubar, 0, s);
}
inline int closure_force(const ins_grid* G, double theta, const double* u, double* sigma, double* m, hipStream_t s) {
  return ins_smagorinsky_force_f64(G, theta, u, sigma, m, s);
}
inline int closure_force(const ins_grid* G, double theta, const float* u, float* sigma, float* m, hipStream_t s) {
  return ins_smagorinsky_force_f32(G, (float)theta, u, sigma, m, s);
}
inline int closure_pullback(const ins_grid* G, double theta, const double* u, const double* sbar, double* ubar, double* thetabar, hipStream_t s) {
  return ins_smagorinsky_force_pullback_f64(G, theta, u, sbar, ubar, 1, thetabar, s);
}
inline int closure_pullback(const ins_grid* G, double theta, const float* u, const float* sbar, float* ubar, double* thetabar, hipStream_t s) {
  return ins_smagorinsky_force_pullback_f32(G, (float)theta, u, sbar, ubar, 1, thetabar, s);
}
inline int temperature_pullback(const ins_grid* G, const ins_temperature_desc_t& td, double visc, const double* u, const double* t, const double* Fbar,
                                const double* cbar, double* ubar, double* tempbar, hipStream_t s) {
  return ins_temperature_pullback_f64(G, &td, visc, u, t, Fbar, cbar, ubar, tempbar, s);
}
inline int temperature_pullback(const ins_grid* G, const ins_temperature_desc_t& td, float visc, const float* u, const float* t, const float* Fbar,
                                const float* cbar, float* ubar, float* tempbar, hipStream_t s) {
  return ins_temperature_pullback_f32(G, &td, visc, u, t, Fbar, cbar, ubar, tempbar, s);
}

// (ubar, tempbar): ∂L/∂(u_out, temp_out) -> ∂L/∂(ustart, tempstart).  with_temp = false: the isothermal step, tempstart and tempbar unused.
template <typename T, typename PS>
int step_pullback(RkAdjointT<T, PS>* adj, bool with_temp, T visc, const T* ustart, const T* tempstart, const T* bodyforce, T dt, T* ubar, T* tempbar,
                  hipStream_t s) {
  const ins_grid* G = adj->grid;
  const int ns = adj->nstage;
  const double* A = adj->A.data();
  const ins_temperature_desc_t& td = adj->td;
  const long long nvec = G->ncell * G->g.D, nsc = with_temp ? G->ncell : 0;
  const size_t sbytes = (size_t)G->ncell * sizeof(T), vbytes = (size_t)nvec * sizeof(T);
  int rc;

  // ---- the stage inputs (v_i, τ_i), the kernel sequence of the reference; k_i lives in y[i], c_i in z[i] until the reverse sweep overwrites them
  INS_HIP_TRY(hipMemcpyAsync(adj->v[0], ustart, vbytes, hipMemcpyDeviceToDevice, s));
  if (with_temp) INS_HIP_TRY(hipMemcpyAsync(adj->tau[0], tempstart, sbytes, hipMemcpyDeviceToDevice, s));
  for (int i = 0; i < ns; ++i) {
    if ((rc = bc_u(G, adj->v[i], s))) return rc;                                              // :19
    if (with_temp && (rc = bc_temp(G, td, adj->tau[i], s))) return rc;                        // :20
    if (i == ns - 1) break;                                                                   // the last k, c enter (u_out, temp_out) only
    if ((rc = momentum(G, visc, adj->v[i], adj->y[i], s))) return rc;                         // :21
    T coef[INS_MAX_STAGES + 1];
    const T* k[INS_MAX_STAGES + 1];
    const bool closure = adj->closure_kind == 1;
    if (with_temp) {
      if ((rc = gravity(G, td, adj->tau[i], adj->y[i], s))) return rc;
      INS_HIP_TRY(hipMemsetAsync(adj->z[i], 0, sbytes, s));                                   // :23-27
      if ((rc = convdiff_temp(G, td, adj->v[i], adj->tau[i], adj->z[i], s))) return rc;
      if (td.dodissipation && (rc = dissipation(G, td, visc, adj->v[i], adj->kbar, adj->z[i], s))) return rc;
      const int n = ins_rk_sum_terms(A, ns, i, dt, adj->z, (const T*)nullptr, coef, k);  // :39-44
      if ((rc = combine(G, G->ncell, tempstart, adj->tau[i + 1], n, coef, k, s))) return rc;
    }
    if (closure) {                                                                            // :31-34, the last term of k_i: k_i += m(v_i, θ)
      if ((rc = closure_force(G, adj->theta, adj->v[i], adj->sigma, adj->mforce, s))) return rc;
      const T one = 1;
      const T* both[1] = {adj->mforce};
      if ((rc = combine(G, nvec, adj->y[i], adj->y[i], 1, &one, both, s))) return rc;
    }
    const int n = ins_rk_sum_terms(A, ns, i, dt, adj->y, bodyforce, coef, k);          // :35-38
    if ((rc = combine(G, nvec, ustart, adj->v[i + 1], n, coef, k, s))) return rc;
    if ((rc = bc_u(G, adj->v[i + 1], s))) return rc;                                          // :48
    if ((rc = project(G, adj->ps, adj->v[i + 1], adj->pwork, s))) return rc;                  // :49
  }

  // ---- reverse sweep.  (g_u, g_T) live in (y[i], z[i]) while they become (ȳ_i, z̄_i); the pullback of stage i writes the next pair into
  // (y[i-1], z[i-1]), the last one into (ubar, tempbar), whose own content has moved to (y[ns-1], z[ns-1]) by then.
  INS_HIP_TRY(hipMemcpyAsync(adj->y[ns - 1], ubar, vbytes, hipMemcpyDeviceToDevice, s));
  if (with_temp) INS_HIP_TRY(hipMemcpyAsync(adj->z[ns - 1], tempbar, sbytes, hipMemcpyDeviceToDevice, s));
  Terms<T> ts;
  for (int i = ns - 1; i >= 0; --i) {
    T* g = adj->y[i];
    if ((rc = bc_u_pullback(G, g, s))) return rc;                                             // :55 (i = ns-1) or :19 of stage i+1
    if ((rc = project_pullback(G, adj->ps, g, adj->pwork, s))) return rc;                     // :49
    if ((rc = bc_u_pullback(G, g, s))) return rc;                                             // :48
    if (with_temp && (rc = bc_temp_pullback(G, td, adj->z[i], s))) return rc;                 // :56 or :20 of stage i+1
    ts.n = 0;
    for (int ip = i; ip < ns; ++ip) {
      const T w = dt * (T)A[ip * ns + i];
      if (w == 0) continue;
      ts.w[ts.n] = w;
      ts.y[ts.n] = adj->y[ip];
      ts.z[ts.n] = with_temp ? adj->z[ip] : nullptr;
      ++ts.n;
    }
    T* out = i > 0 ? adj->y[i - 1] : ubar;
    T* tout = with_temp ? (i > 0 ? adj->z[i - 1] : tempbar) : nullptr;
    if (ts.n == 0) {
      INS_HIP_TRY(hipMemsetAsync(out, 0, vbytes, s));
      if (with_temp) INS_HIP_TRY(hipMemsetAsync(tout, 0, sbytes, s));
      continue;
    }
    if ((rc = launch_sums<T, false>(nvec, nsc, adj->kbar, adj->cbar, ts, s))) return rc;
    if ((rc = momentum_pullback(G, visc, adj->v[i], adj->kbar, out, s))) return rc;
    if (adj->closure_kind == 1 && (rc = closure_pullback(G, adj->theta, adj->v[i], adj->kbar, out, adj->thetabar, s))) return rc;
    if (with_temp && (rc = temperature_pullback(G, td, visc, adj->v[i], adj->tau[i], adj->kbar, adj->cbar, out, tout, s))) return rc;
  }
  if ((rc = bc_u_pullback(G, ubar, s))) return rc;                                            // :19 of stage 0
  if (with_temp && (rc = bc_temp_pullback(G, td, tempbar, s))) return rc;                     // :20 of stage 0
  ts.n = ns;
  for (int i = 0; i < ns; ++i) {
    ts.w[i] = 1;
    ts.y[i] = adj->y[i];
    ts.z[i] = with_temp ? adj->z[i] : nullptr;
  }
  return launch_sums<T, true>(nvec, nsc, ubar, tempbar, ts, s);
}

}  // namespace rkadj
