// Gather kernels of the temperature equation's pullbacks (operators.jl:712-737, 791-814, 884-931; boundary_conditions.jl:236-270, 338-342,
// 391-412, 466-470, 512-516), once for both precisions: templates over the scalar type T of the fields, instantiated with double by
// ins_temp_adjoint.hip and with float by ins_temp_adjoint32.hip (two translation units, so that each keeps its register allocation).  Each
// is the exact transpose of THIS library's forward operator on the whole padded arrays (DESIGN.md "Differentiability", "Temperature
// equation"): of k_bc_temp, k_gravity and k_dissipation_interp (ins_temp_kernels.h, both precisions), with T = double of k_convdiff_temp and
// diffusion (ins_fields.hip, ins_operators.hip), with T = float of k32t_convdiff_temp and k32t_diffusion (ins_temp32.hip).
// The reference's own rules stop short here: the rrule of convection_diffusion_temp returns undefined names (operators.jl:699-704) and
// dissipation's is @test_broken; only gravity and apply_bc_temp have working pullbacks.
//
// Gather form as in ins_adjoint_kernels.h: one work-item per volume of the padded array reads the cotangent stencil around it, every output
// is written once by one work-item, no atomics, so every result is bitwise reproducible.  2-D and 3-D, any BC mix, uniform and stretched
// grids.  One kernel template serves the four operator-level entries and the fused per-stage entry: PARTS selects the terms, so the fused
// launch forms exactly the sums of the operator-level ones.
//
// The one rule for both precisions (ins_adjoint_kernels.h): the grid handle is the fp64 one, a metric table entry is read as a double and
// converted with (T) where it enters the arithmetic, constants are written T(…), and everything else is in T.  With T = double the
// conversions vanish.  With T = float the weights are formed as the Float32 forward forms them — (float)Δ first, then d1 / (d0 + d1) in
// float, as avg_at<float> and avg32 — so the pullback is the transpose of the Float32 operator up to float rounding, not the fp64 transpose rounded at the end.
//
// A face is evaluated only where the forward evaluated it: the in_ip / in_iu / dof masks are branches around the reads, never factors.  A
// zero-width ghost volume has Δ = eps(Float64), so 1/Δ ≈ 4.5e15: finite in float, and so is the product of two such entries, but a masked-out
// face times a zero cotangent would be 0 · inf as soon as one more factor came in.
#pragma once

#include "ins_stencil.h"

namespace {

// --------------------------------------------------------------------------------------------
// gravity_adjoint                                                        operators.jl:892-908
//   forward: F[J, g] += α2 avg(temp, J, g), J ∈ Iu[g], avg(ϕ, J, g) = (Δ[Jg+1] ϕ[J] + Δ[Jg] ϕ[J+eg]) / (Δ[Jg] + Δ[Jg+1])   (avg_at)
//   tempbar[K] gets α2 (φ[K] Δ[Kg+1]/(Δ[Kg]+Δ[Kg+1]) [K ∈ Iu[g]] + φ[K−eg] Δ[Kg−1]/(Δ[Kg−1]+Δ[Kg]) [K−eg ∈ Iu[g]])
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__device__ __forceinline__ T gravity_tempbar(const GridDev& g, int gdir, T a2, const T* __restrict__ phig, const int (&I)[3], long long c) {
  const int ig = I[gdir];
  const double* dx = g.dx[gdir];
  T v = T(0.0);
  if (in_iu<D>(g, gdir, I[0], I[1], I[2])) {
    const T d0 = (T)dx[ig], d1 = (T)dx[ig + 1];
    v += phig[c] * (d1 / (d0 + d1));
  }
  if (in_iu<D>(g, gdir, INS_SH(I, gdir, -1))) {
    const T d0 = (T)dx[ig - 1], d1 = (T)dx[ig];
    v += phig[c - g.sx[gdir]] * (d0 / (d0 + d1));
  }
  return a2 * v;
}

// --------------------------------------------------------------------------------------------
// convection_diffusion_temp_adjoint                                      operators.jl:712-737
//   forward, I ∈ Ip:  c[I] += Σ_β [ −(uβ[I] avg(T, I, β) − uβ[I−eβ] avg(T, I−eβ, β)) + α4 ((T[I+eβ] − T[I])/Δuβ[Iβ] − (T[I] − T[I−eβ])/Δuβ[Iβ−1]) ] / Δβ[Iβ]
//   With q = cbar masked to Ip, the flux uβ[J] avg(T, J, β) through the upper β-face of J carries ψβ(J) = q[J+eβ]/Δβ[Jβ+1] − q[J]/Δβ[Jβ]:
//     ubar[J, β]  gets avg(T, J, β) ψβ(J)
//     tempbar[K]  gets Σ_β uβ[K] ψβ(K) Δ[Kβ+1]/(Δ[Kβ]+Δ[Kβ+1]) + uβ[K−eβ] ψβ(K−eβ) Δ[Kβ−1]/(Δ[Kβ−1]+Δ[Kβ])       (the two averages that read T[K])
//                 + α4 Σ_β ( q[K−eβ]/(Δβ Δuβ)[Kβ−1] − q[K] (1/Δuβ[Kβ] + 1/Δuβ[Kβ−1])/Δβ[Kβ] + q[K+eβ]/(Δβ[Kβ+1] Δuβ[Kβ]) )
//   A face is evaluated only where ψ has a term, i.e. exactly where the forward evaluated it, so every table and field read is one the
//   forward made (no 0 · inf from a zero-width ghost volume, no read outside the array).
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__device__ __forceinline__ T cdt_tempbar(const GridDev& g, T a4, const T* __restrict__ u, const T* __restrict__ cbar, const int (&I)[3],
                                         long long c) {
  const bool here = in_ip<D>(g, I[0], I[1], I[2]);
  const T qc = here ? cbar[c] : T(0.0);
  T v = T(0.0);
#pragma unroll
  for (int b = 0; b < D; ++b) {
    const long long sb = g.sx[b];
    const int ib = I[b];
    const T* ub = u + b * g.sc;
    const double* dx = g.dx[b];
    const double* rdx = g.rdx[b];
    const double* rdxu = g.rdxu[b];
    const bool up = in_ip<D>(g, INS_SH(I, b, 1)), dn = in_ip<D>(g, INS_SH(I, b, -1));
    const T qp = up ? cbar[c + sb] : T(0.0), qm = dn ? cbar[c - sb] : T(0.0);
    if (here || up) {  // face of K
      T psi = T(0.0);
      if (up) psi += qp * (T)rdx[ib + 1];
      if (here) psi -= qc * (T)rdx[ib];
      const T d0 = (T)dx[ib], d1 = (T)dx[ib + 1];
      v += ub[c] * psi * (d1 / (d0 + d1));
    }
    if (dn || here) {  // face of K − eβ
      T psi = T(0.0);
      if (here) psi += qc * (T)rdx[ib];
      if (dn) psi -= qm * (T)rdx[ib - 1];
      const T d0 = (T)dx[ib - 1], d1 = (T)dx[ib];
      v += ub[c - sb] * psi * (d0 / (d0 + d1));
    }
    if (dn) v += a4 * qm * (T)rdx[ib - 1] * (T)rdxu[ib - 1];
    if (here) v -= a4 * qc * (T)rdx[ib] * ((T)rdxu[ib] + (T)rdxu[ib - 1]);
    if (up) v += a4 * qp * (T)rdx[ib + 1] * (T)rdxu[ib];
  }
  return v;
}

template <int D, typename T>
__device__ __forceinline__ T cdt_ubar(const GridDev& g, int b, const T* __restrict__ temp, const T* __restrict__ cbar, const int (&I)[3],
                                      long long c) {
  const bool here = in_ip<D>(g, I[0], I[1], I[2]);
  const bool up = in_ip<D>(g, INS_SH(I, b, 1));
  if (!(here || up)) return T(0.0);
  const int ib = I[b];
  T psi = T(0.0);
  if (up) psi += cbar[c + g.sx[b]] * (T)g.rdx[b][ib + 1];
  if (here) psi -= cbar[c] * (T)g.rdx[b][ib];
  const T d0 = (T)g.dx[b][ib], d1 = (T)g.dx[b][ib + 1];
  return psi * ((d1 * temp[c] + d0 * temp[c + g.sx[b]]) / (d0 + d1));
}

// --------------------------------------------------------------------------------------------
// dissipation_adjoint                                                    operators.jl:791-814
//   forward: d = diffusion(u) on the degrees of freedom of u and zero elsewhere (fill! + diffusion!, :797-798), then for I ∈ Ip
//     φ[I] += coef Σ_β (uβ[I−eβ] dβ[I−eβ] + uβ[I] dβ[I]) / 2.
//   With wbar[J, γ] = coef/2 (q[J] + q[J+eγ]) [J dof of γ], q = cbar masked to Ip:
//     ubar[J, γ] gets wbar[J, γ] dγ[J] + (diffusionᵀ z)[J, γ],   z = wbar ⊙ u.
//   d and z are recomputed from their stencils (no D-component scratch field); the ranges (dof) and boundary-volume widths (mdx / mdxu, r) are
//   those of k_convdiff (ins_diffusion_f64) and k32t_diffusion, and of k_convdiff_adjoint (ins_diffusion_adjoint_f64).
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__device__ __forceinline__ T diss_z(const GridDev& g, T halfcoef, int ga, const T* __restrict__ ua, const T* __restrict__ cbar, int i0, int i1,
                                    int i2, long long c) {
  T q = T(0.0);
  if (in_ip<D>(g, i0, i1, i2)) q += cbar[c];
  if (in_ip<D>(g, i0 + (ga == 0), i1 + (ga == 1), i2 + (ga == 2))) q += cbar[c + g.sx[ga]];
  return halfcoef * q * ua[c];
}

template <int D, typename T>
__device__ __forceinline__ T diss_ubar(const GridDev& g, T visc, T coef, int ga, const T* __restrict__ u, const T* __restrict__ cbar,
                                       const int (&I)[3], long long c) {
  const T* ua = u + ga * g.sc;
  const T hc = T(0.5) * coef;
  const bool dx = dof<D>(g, ga, I[0], I[1], I[2]);
  T v = T(0.0);
  T zc = T(0.0);
  if (dx) {
    const T uc = ua[c];
    T q = T(0.0);
    if (in_ip<D>(g, I[0], I[1], I[2])) q += cbar[c];
    if (in_ip<D>(g, INS_SH(I, ga, 1))) q += cbar[c + g.sx[ga]];
    const T wb = hc * q;
    zc = wb * uc;
    T d = T(0.0);
#pragma unroll
    for (int be = 0; be < D; ++be) {
      const long long sb = g.sx[be];
      const int ib = I[be];
      const T r = (T)(ga == be ? g.rdxu[be] : g.rdx[be])[ib];
      const T ma = (T)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
      const T mb = (T)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
      d += visc * ((ua[c + sb] - uc) * mb - (uc - ua[c - sb]) * ma) * r;
    }
    v += wb * d;
  }
#pragma unroll
  for (int be = 0; be < D; ++be) {
    const long long sb = g.sx[be];
    const int ib = I[be];
    const double* rt = ga == be ? g.rdxu[be] : g.rdx[be];
    if (dx) {
      const T ma = (T)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
      const T mb = (T)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
      v -= visc * zc * (T)rt[ib] * (ma + mb);
    }
    if (dof<D>(g, ga, INS_SH(I, be, -1))) {
      const T mb = (T)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
      v += visc * diss_z<D, T>(g, hc, ga, ua, cbar, INS_SH(I, be, -1), c - sb) * (T)rt[ib - 1] * mb;
    }
    if (dof<D>(g, ga, INS_SH(I, be, 1))) {
      const T ma = (T)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
      v += visc * diss_z<D, T>(g, hc, ga, ua, cbar, INS_SH(I, be, 1), c + sb) * (T)rt[ib + 1] * ma;
    }
  }
  return v;
}

// PARTS bit0: gravityᵀ -> tempbar   bit1: (∂c/∂temp)ᵀ -> tempbar   bit2: (∂c/∂u)ᵀ -> ubar   bit3: dissipationᵀ -> ubar
// TOVER: tempbar is overwritten, else added to.  ubar is always added to.
enum { P_GRAV = 1, P_CDT_T = 2, P_CDT_U = 4, P_DISS = 8 };
template <typename T>
struct TempAdjArgs {
  int gdir;
  T a2, a4, visc, coef;
  const T* u;
  const T* temp;
  const T* Fbar;
  const T* cbar;
  T* ubar;
  T* tempbar;
};

template <int D, typename T, int PARTS, bool TOVER>
__global__ __launch_bounds__(256) void k_temp_adjoint(GridDev g, BoxMap L, TempAdjArgs<T> a) {
  INS_BANDED_INDEX(0, 0, 0, g.N[0], g.N[1]);
  if (PARTS & (P_GRAV | P_CDT_T)) {
    T v = T(0.0);
    if (PARTS & P_GRAV) v += gravity_tempbar<D, T>(g, a.gdir, a.a2, a.Fbar + a.gdir * g.sc, I, c);
    if (PARTS & P_CDT_T) v += cdt_tempbar<D, T>(g, a.a4, a.u, a.cbar, I, c);
    a.tempbar[c] = TOVER ? v : a.tempbar[c] + v;
  }
  if (PARTS & (P_CDT_U | P_DISS)) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
      T v = T(0.0);
      if (PARTS & P_CDT_U) v += cdt_ubar<D, T>(g, b, a.temp, a.cbar, I, c);
      if (PARTS & P_DISS) v += diss_ubar<D, T>(g, a.visc, a.coef, b, a.u, a.cbar, I, c);
      a.ubar[b * g.sc + c] += v;
    }
  }
}

template <typename T, int PARTS, bool TOVER>
int launch_temp_adjoint(const ins_grid* G, const TempAdjArgs<T>& a, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = banded_launch(g.D, g.N);
  INS_LAUNCH_D((k_temp_adjoint<D, T, PARTS, TOVER>), l, s, g, l.map, a);
  return INS_OK;
}

// --------------------------------------------------------------------------------------------
// apply_bc_temp_pullback         boundary_conditions.jl:142-157, 248-270, 341-342, 407-412, 469-470, 515-516
//   The exact transpose of k_bc_temp (ins_temp_kernels.h): the forward sweeps β = 0..D-1 and fills, per line,
//   the left then the right ghost volume with a copy (x[i] = x[j]) or a Dirichlet value; the transpose walks β = D-1..0 and the sides right
//   then left, turning x[i] = x[j] into (x̄[j] += x̄[i]; x̄[i] = 0) and x[i] = value into x̄[i] = 0.  The Dirichlet values (constant or
//   callable) only change the constant part, so neither they nor t enter.
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_temp_pullback(GridDev g, T* __restrict__ tb, int be, int bcl, int bcr) {
  INS_LINE_INDEX(be);
  T* x = tb + base;
  const long long sb = g.sx[be];
  const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
  if (bcl == INS_BC_PERIODIC) {  // forward: x[ia] = x[ib-1]; x[ib] = x[ia+1]
    move_to(x, ib * sb, (ia + 1) * sb);
    move_to(x, ia * sb, (ib - 1) * sb);
    return;
  }
#pragma unroll
  for (int side = 1; side >= 0; --side) {
    const int bc = side ? bcr : bcl;
    const int i = side ? ib : ia;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_DIRICHLET)
      x[i * sb] = T(0.0);
    else if (bc == INS_BC_SYMMETRIC || bc == INS_BC_PRESSURE)
      move_to(x, i * sb, jn * sb);
  }
}

// The BC-code checks of the ghost-fill pullback entries (those of ins_apply_bc_temp_f64 / _f32), then the sweep in reverse direction order
template <typename T>
int bc_temp_pullback(const ins_grid* G, const int32_t* bc, T* tempbar, hipStream_t s) {
  const GridDev& g = G->g;
  for (int be = 0; be < g.D; ++be) {
    for (int side = 0; side < 2; ++side) {
      const int c = bc[2 * be + side];
      INS_REQUIRE(c == INS_BC_PERIODIC || c == INS_BC_DIRICHLET || c == INS_BC_SYMMETRIC || c == INS_BC_PRESSURE, "temperature boundary condition");
    }
    INS_REQUIRE((bc[2 * be] == INS_BC_PERIODIC) == (bc[2 * be + 1] == INS_BC_PERIODIC), "periodic on both sides");
  }
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_apply_bc_temp_f64 / _f32
    INS_LAUNCH_D((k_bc_temp_pullback<D, T>), line_launch(g, be, 1), s, g, tempbar, be, (int)bc[2 * be], (int)bc[2 * be + 1]);
  }
  return INS_OK;
}

}  // namespace
