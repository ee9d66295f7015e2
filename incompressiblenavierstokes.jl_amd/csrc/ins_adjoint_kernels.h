// Gather kernels of the step pullbacks (operators.jl:100-616, boundary_conditions.jl:114-230, 290-516), once for both precisions: templates
// over the scalar type T of the fields, instantiated with double by ins_adjoint.hip and with float by ins_adjoint32.hip (two translation
// units, so that each keeps its register allocation).  Each kernel is the exact transpose of this library's forward operator on the whole
// padded array, ghost volumes included (DESIGN.md "Differentiability"): one work-item per output volume reads the cotangent stencil around
// it, so no atomics and every output is written once.  2-D and 3-D, any BC mix, uniform and stretched grids.
//
// The one rule for both precisions: the grid handle is the fp64 one, a metric table entry is read as a double and converted with (T) where
// it enters the arithmetic, constants are written T(…), and everything else is in T.  With T = double the conversions vanish and the
// expressions are those of the generic forward operators.  The forward twins: ins_operator_kernels.h (k_divergence, k_bc_u, k_bc_p, both
// precisions) and, for the two stencils whose precisions contract their FMAs differently, k_convdiff / k_pressuregradient in
// ins_operators.hip with the float copies k32g_momentum / k32g_applypressure in ins_f32g.hip.
#pragma once

#include "ins_stencil.h"

namespace {

// --------------------------------------------------------------------------------------------
// divergence_adjoint                                                     operators.jl:127-145
//   ubar[α][I] += alpha · (φ[I]/Δα[Iα] [I ∈ Ip] − φ[I+eα]/Δα[Iα+1] [I+eα ∈ Ip])   over the whole padded array
//   φ and alpha have type P, ubar type T: the sum is taken in P and rounded to T once.  <double, float>: φ is the pressure of the fp64
//   solver that a Float32 solver handle wraps (the mirror of k_divergence<D, float, double, true>, which forms that solver's right-hand side in double
//   from the float field).
// --------------------------------------------------------------------------------------------
template <int D, typename P, typename T>
__global__ __launch_bounds__(256) void k_divergence_adjoint(GridDev g, const P* __restrict__ phi, T* __restrict__ ubar, P alpha) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  const bool here = in_ip<D>(g, i, j, k);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    P v = 0;
    if (here) v += phi[c] * (P)g.rdx[a][I[a]];
    if (in_ip<D>(g, INS_SH(I, a, 1))) v -= phi[c + g.sx[a]] * (P)g.rdx[a][I[a] + 1];
    ubar[a * g.sc + c] += (T)(alpha * v);
  }
}

// --------------------------------------------------------------------------------------------
// pressuregradient_adjoint                                               operators.jl:180-199
//   pbar[I] += Σα (φα[I−eα]/Δuα[Iα−1] [I−eα dof of α] − φα[I]/Δuα[Iα] [I dof of α])
//   φ has type T, pbar type P, the sum is taken in P.  ACC = false writes every volume of the padded array: <float, double, false> forms
//   the wrapped solver's fp64 right-hand side Gᵀφ in double from the float cotangent.
// --------------------------------------------------------------------------------------------
template <int D, typename T, typename P, bool ACC>
__global__ __launch_bounds__(256) void k_pressuregradient_adjoint(GridDev g, const T* __restrict__ phi, P* __restrict__ pbar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  P v = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* pa = phi + a * g.sc;
    if (dof<D>(g, a, i, j, k)) v -= (P)pa[c] * (P)g.rdxu[a][I[a]];
    if (dof<D>(g, a, INS_SH(I, a, -1))) v += (P)pa[c - g.sx[a]] * (P)g.rdxu[a][I[a] - 1];
  }
  pbar[c] = ACC ? pbar[c] + v : v;
}

// --------------------------------------------------------------------------------------------
// convection / diffusion pullback                               operators.jl:417-519, 575-616
//   The forward (k_convdiff, k32g_momentum) adds to a DOF volume c of component α, per direction β,
//     r(c)·[ ν(mb(c)(u[c+eβ]−u[c]) − ma(c)(u[c]−u[c−eβ])) − (Φ(c) − Φ(c−eβ)) ],
//     Φ(f) = ½(uα[f]+uα[f+eβ]) · (A₂βα[fα] uβ[f] + A₁βα[fα+1] uβ[f+eα])        (the flux through the upper β-face of f)
//   with r = 1/Δuβ (α == β) or 1/Δβ.  So ⟨φ, F⟩ = Σ_f ψ(f) Φ(f) + diffusion terms with
//     ψαβ(f) = −r(f) φα[f] [f dof] + r(f+eβ) φα[f+eβ] [f+eβ dof],
//   and ubar = J(u)ᵀφ gathers, per output volume x and component γ:
//     (a) α = γ:  ψγβ(f) · ½(A₂ uβ[f] + A₁ uβ[f+eγ])         for f = x and f = x − eβ
//     (b) β = γ:  ψαγ(x) · ½(uα[x]+uα[x+eγ]) · A₂γα[xα]    and  ψαγ(x−eα) · ½(uα[x−eα]+uα[x−eα+eγ]) · A₁γα[xα]
//   (both when α = β = γ: the product rule).  A flux is evaluated only where ψ has a DOF term, i.e. exactly where the
//   forward evaluated it, so every read stays inside the padded array.
//   MODE bit0 = convection, bit1 = diffusion (3: the momentum pullback).  ACC: ubar += J^T φ, else ubar = J^T φ.
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__device__ __forceinline__ T rr(const GridDev& g, int al, int be, int ib) {
  return (T)(al == be ? g.rdxu[be] : g.rdx[be])[ib];
}

// ψαβ(f) at f = (f0, f1, f2) (linear index cf); `live` = it has a DOF term
template <int D, typename T, typename PA>
__device__ __forceinline__ T psi(const GridDev& g, int al, int be, const int (&F)[3], long long cf, PA phia, bool& live) {
  const bool d0 = dof<D>(g, al, F[0], F[1], F[2]);
  const bool d1 = dof<D>(g, al, INS_SH(F, be, 1));
  live = d0 || d1;
  T v = T(0);
  if (d0) v -= rr<D, T>(g, al, be, F[be]) * phia[cf];
  if (d1) v += rr<D, T>(g, al, be, F[be] + 1) * phia[cf + g.sx[be]];
  return v;
}

// The cotangent φ is read through phi_comp(φ, component offset)[volume]: an array (const T*), or a PhiComb, the combination Σ_q w[q]·p[q] of up to
// S arrays formed where it is read.  The reverse Runge-Kutta stage (ins_rk_adjoint.hip) takes the second: its φ is k̄_i = Δt Σ_{i'≥i} A[i',i] ȳ_{i'},
// which then is never written to memory (one write and one read of a vector field less per stage; the stencil's repeated reads hit the cache, but
// re-forming the sum at every stencil point costs more than the traffic saved: opt-in, INS_ADJ_STAGE_FUSED=1).
constexpr int INS_ADJ_COMB_MAX = 4;  // arrays of a combined cotangent in the instantiations (RK44's first reverse stage has 4); longer sums go through memory

template <typename T, int S>
struct PhiComb {
  const T* p[S];
  T w[S];
  int n;
};

template <typename T, int S>
struct PhiCombAt {
  const PhiComb<T, S>& a;
  long long off;
  __device__ __forceinline__ T operator[](long long idx) const {
    T v = T(0);
#pragma unroll
    for (int q = 0; q < S; ++q)
      if (q < a.n) v += a.w[q] * a.p[q][off + idx];
    return v;
  }
};

template <typename T>
__device__ __forceinline__ const T* phi_comp(const T* phi, long long off) {
  return phi + off;
}
template <typename T, int S>
__device__ __forceinline__ PhiCombAt<T, S> phi_comp(const PhiComb<T, S>& phi, long long off) {
  return PhiCombAt<T, S>{phi, off};
}

// the kernel parameter of a cotangent source: a restrict-qualified pointer, as before the source became a template parameter, or the PhiComb by value
template <typename Phi>
struct PhiParam {
  using type = Phi;
};
template <typename T>
struct PhiParam<const T*> {
  using type = const T* __restrict__;
};

template <int D, typename T, int MODE, bool ACC, typename Phi = const T*>
__global__ __launch_bounds__(256) void k_convdiff_adjoint(GridDev g, T visc, const T* __restrict__ u, typename PhiParam<Phi>::type phi, T* __restrict__ ubar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);

#pragma unroll
  for (int ga = 0; ga < D; ++ga) {
    const auto pg = phi_comp(phi, ga * g.sc);
    T v = T(0);
    if (MODE & 2) {
      const bool dx = dof<D>(g, ga, i, j, k);
#pragma unroll
      for (int be = 0; be < D; ++be) {
        const int ib = I[be];
        const long long sb = g.sx[be];
        // ma(i) = mdx[i] | mdxu[i-1],  mb(i) = mdx[i+1] | mdxu[i]   (k_convdiff)
        if (dx) {
          const T ma = (T)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
          const T mb = (T)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
          v -= visc * pg[c] * rr<D, T>(g, ga, be, ib) * (ma + mb);
        }
        if (dof<D>(g, ga, INS_SH(I, be, -1))) {
          const T mb = (T)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
          v += visc * pg[c - sb] * rr<D, T>(g, ga, be, ib - 1) * mb;
        }
        if (dof<D>(g, ga, INS_SH(I, be, 1))) {
          const T ma = (T)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
          v += visc * pg[c + sb] * rr<D, T>(g, ga, be, ib + 1) * ma;
        }
      }
    }
    if (MODE & 1) {
      const long long sg = g.sx[ga];
      // (a) α = γ: ∂Φγβ(f)/∂uγ = ½ (A₂βγ[fγ] uβ[f] + A₁βγ[fγ+1] uβ[f+eγ])
#pragma unroll
      for (int be = 0; be < D; ++be) {
        const long long sb = g.sx[be];
        const T* ub = u + be * g.sc;
        const double* A1 = g.A1[be][ga];
        const double* A2 = g.A2[be][ga];
#pragma unroll
        for (int sh = 0; sh < 2; ++sh) {  // f = x, x − eβ
          const int F[3] = {INS_SH(I, be, -sh)};
          const long long cf = c - sh * sb;
          bool live;
          const T w = psi<D, T>(g, ga, be, F, cf, pg, live);
          if (live) v += w * T(0.5) * ((T)A2[F[ga]] * ub[cf] + (T)A1[F[ga] + 1] * ub[cf + sg]);
        }
      }
      // (b) β = γ: ∂Φαγ(f)/∂uγ[f] = ½(uα[f]+uα[f+eγ]) A₂γα[fα];  ∂Φαγ(f)/∂uγ[f+eα] = ½(uα[f]+uα[f+eγ]) A₁γα[fα+1]
#pragma unroll
      for (int al = 0; al < D; ++al) {
        const long long sa = g.sx[al];
        const T* ua = u + al * g.sc;
        const auto pa = phi_comp(phi, al * g.sc);
        const double* A1 = g.A1[ga][al];
        const double* A2 = g.A2[ga][al];
        {
          bool live;
          const T w = psi<D, T>(g, al, ga, I, c, pa, live);
          if (live) v += w * T(0.5) * (ua[c] + ua[c + sg]) * (T)A2[I[al]];
        }
        {
          const int F[3] = {INS_SH(I, al, -1)};
          const long long cf = c - sa;
          bool live;
          const T w = psi<D, T>(g, al, ga, F, cf, pa, live);
          if (live) v += w * T(0.5) * (ua[cf] + ua[cf + sg]) * (T)A1[I[al]];
        }
      }
    }
    T* ob = ubar + ga * g.sc + c;
    *ob = ACC ? *ob + v : v;
  }
}

// --------------------------------------------------------------------------------------------
// apply_bc_u_pullback / apply_bc_p_pullback           boundary_conditions.jl:169-230, 290-516
//   The exact transpose of k_bc_u / k_bc_p (ins_operator_kernels.h, both precisions; and, on periodic boxes, of k32_bc_periodic, which
//   does the same copies): the forward sweeps β = 0..D-1 and, per line, left side then right side, each fill a copy (x[i] = x[j]) or a
//   constant; the transpose walks β = D-1..0 and the sides right then left, turning x[i] = x[j] into (x̄[j] += x̄[i]; x̄[i] = 0) and
//   x[i] = const into x̄[i] = 0.  Time-dependent Dirichlet planes only change the constant, so the pullback does not read them.
//   A slab (HALO) side is not a boundary and is skipped; the Float32 entries reject such grids before they launch.
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_u_pullback(GridDev g, T* __restrict__ u, int be) {
  INS_LINE_INDEX(be);
  const int al = blockIdx.z;
  const long long sb = g.sx[be];
  T* ua = u + al * g.sc + base;
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  if (bcl == INS_BC_PERIODIC) {  // forward: x[ia] = x[ib-1]; x[ib] = x[ia+1]
    const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
    move_to(ua, ib * sb, (ia + 1) * sb);
    move_to(ua, ia * sb, (ib - 1) * sb);
    return;
  }
#pragma unroll
  for (int side = 1; side >= 0; --side) {
    const int bc = side ? bcr : bcl;
    if (bc == INS_BC_HALO) continue;
    const int i = side ? g.iu_hi[al][be] : g.iu_lo[al][be] - 1;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_DIRICHLET || (bc == INS_BC_SYMMETRIC && al == be))
      ua[i * sb] = T(0);
    else if (bc == INS_BC_SYMMETRIC || bc == INS_BC_PRESSURE)
      move_to(ua, i * sb, jn * sb);
  }
}

template <int D, typename T>
__global__ __launch_bounds__(256) void k_bc_p_pullback(GridDev g, T* __restrict__ p, int be) {
  INS_LINE_INDEX(be);
  T* pl = p + base;
  const long long sb = g.sx[be];
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
  if (bcl == INS_BC_PERIODIC) {
    move_to(pl, ib * sb, (ia + 1) * sb);
    move_to(pl, ia * sb, (ib - 1) * sb);
    return;
  }
#pragma unroll
  for (int side = 1; side >= 0; --side) {
    const int bc = side ? bcr : bcl;
    const int i = side ? ib : ia;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_SYMMETRIC)
      move_to(pl, i * sb, jn * sb);
    else if (bc == INS_BC_PRESSURE)
      pl[i * sb] = T(0);
  }
}

}  // namespace
