// Pullback of the Smagorinsky closure force once for both precisions, as templates over the scalar type T of the fields:
// ins_smagpullback.hip instantiates them with double, ins_smagpullback32.hip with float.
//
// Forward, at a ghost-filled u (operators.jl:1135-1150, 1203-1236, 1284-1300):
//   σ = 2 νt S on Ip,  νt = θ² Δ² |S|,  |S| = sqrt(2 S:S),  S = sym ∇u,  Δ² = Σ Δα²;   apply_bc_p on every component of σ;   s = divoftensor(σ) on Iu[α].
// Pullback of (u, θ) for a cotangent s̄ (read on Iu[α] only), pass 1, one work-item per pressure point I:
//   σ̄(I) = Σ_{J ∈ images(I)} (divoftensorᵀ s̄)(J).  apply_bc_p fills direction by direction over whole padded planes, and the source index of a ghost
//   index depends on that direction's coordinate alone, so the volumes that hold a copy of σ(I) are the product over the directions of
//   {I_β} ∪ {ghost indices of β whose source is I_β}: the periodic image(s), the ghost next to a Symmetric side, nothing at a Dirichlet side (left as
//   allocated) or a Pressure side (set to zero).  σ̄ stays in registers.
//   With M the symmetric matrix of σ̄ (<M, B> = Σ_{a<=b} σ̄_ab B_ab) and c = θ²Δ²:  dσ = 2c (|S| dS + 2 S (S:dS) / |S|), so
//     Ḡ = 2c (|S| M + 2 (M:S) / |S| · S)   (symmetric; zero where |S| = 0),   and   <σ̄, σ̂> = 2 Δ² |S| (M:S)  at θ = 1  (σ = θ² σ̂, θbar = 2θ Σ_I <σ̄, σ̂>).
//   Ḡ goes to the grid handle's ∇ubar scratch (field a·D + b), the cell's term of <σ̄, σ̂> is reduced over the workgroup in double in a fixed
//   order and written as one partial per workgroup.
// Pass 2 is the transpose-of-∇ gather of the tensor-basis pullbacks (k_gradu_adjoint, ins_tensorclosure.hip, and its float copy).  The tail,
// k_smag_thetabar, sums the partials in a fixed order in double and adds 2θ·sum to a device double.  No atomic operations: results are bitwise
// reproducible from run to run.
//
// ∇u is that of strain_rotation (ins_tensorbasis.h), the four one-sided differences of an off-diagonal entry with the stretched metrics.  On an
// exactly uniform box (UNI) they share their metric and the middle values cancel: two central differences, as in k_smagforce, whose header says why
// (instruction issue, not HBM, bounds these kernels).
#pragma once

#include "ins_tensorbasis.h"

namespace {

// (divoftensorᵀ s̄)(J), added to t[sym_index]: the expressions of k_divoftensor_adjoint (ins_tensorclosure.hip) at one volume J of the padded array.
// The masks are true only for volumes inside the array, so a J on the array's edge reads nothing outside it.
template <int D, typename T>
__device__ __forceinline__ void sigbar_at(const GridDev& g, const T* __restrict__ sbar, const int (&J)[3], T (&t)[D * (D + 1) / 2]) {
  const long long cj = J[0] + J[1] * g.sx[1] + (D == 3 ? J[2] * g.sx[2] : 0);
  auto w = [&](int al, int be, int dal, int dbe) -> T {
    int K[3] = {J[0], J[1], J[2]};
    K[al] += dal;
    K[be] += dbe;
    if (!in_iu<D>(g, al, K[0], K[1], K[2])) return T(0);
    return sbar[al * g.sc + cj + dal * g.sx[al] + dbe * g.sx[be]] * (T)g.rdx[be][K[be]] / 4;
  };
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      T v = T(0);
      if (a == b) {
        if (in_iu<D>(g, a, INS_SH(J, a, -1))) v += sbar[a * g.sc + cj - g.sx[a]] * (T)g.rdxu[a][J[a] - 1];
        if (in_iu<D>(g, a, J[0], J[1], J[2])) v -= sbar[a * g.sc + cj] * (T)g.rdxu[a][J[a]];
      } else {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int al = q ? b : a, be = q ? a : b;
          v += w(al, be, 0, -1) + w(al, be, -1, -1) - w(al, be, 0, 1) - w(al, be, -1, 1);
        }
      }
      t[sym_index<D>(a, b)] += v;
    }
}

// The ghost indices of direction b that apply_bc_p fills from the pressure point index Ib (k_bc_p, ins_operator_kernels.h): n of them in gh[0..n-1]
__device__ __forceinline__ int ghost_images(const GridDev& g, int b, int Ib, int (&gh)[2]) {
  const int bcl = g.bc[b][0], bcr = g.bc[b][1];
  const int ia = g.ip_lo[b] - 1, ib = g.ip_hi[b];
  int n = 0;
  if (bcl == INS_BC_PERIODIC) {  // p[ia] = p[ib-1]; p[ib] = p[ia+1]
    if (Ib == ib - 1) gh[n++] = ia;
    if (Ib == ia + 1) gh[n++] = ib;
  } else {  // Symmetric: p[ia] = p[ia+1], p[ib] = p[ib-1]; Dirichlet: untouched; Pressure: zero; a slab's halo sides are refused by the entry
    if (bcl == INS_BC_SYMMETRIC && Ib == ia + 1) gh[n++] = ia;
    if (bcr == INS_BC_SYMMETRIC && Ib == ib - 1) gh[n++] = ib;
  }
  return n;
}

// S = sym ∇u at the pressure point on an exactly uniform box: an off-diagonal entry from two central differences
template <int D, typename T>
__device__ __forceinline__ void strain_uniform(const GridDev& g, const T* __restrict__ u, long long c, const int (&I)[3], Mat<D, T>& S) {
  T G[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* ua = u + a * g.sc;
    const long long sa = g.sx[a];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      if (a == b)
        G[a][b] = (ua[c] - ua[c - sb]) * (T)g.rdx[b][I[b]];
      else
        G[a][b] = ((ua[c + sb] - ua[c - sb]) + (ua[c - sa + sb] - ua[c - sa - sb])) * ((T)g.rdxu[b][I[b]] / 4);
    }
  }
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) S.m[a][b] = (G[a][b] + G[b][a]) / 2;
}

// pass 1.  The launch covers Ip in 64x4 tiles; a work-item outside Ip (ragged last tiles) contributes zero to the workgroup's partial and
// stays for the barrier.  part == nullptr: no θ cotangent is asked for, no reduction.
template <int D, typename T, bool UNI>
__global__ __launch_bounds__(256) void k_smag_gradbar(GridDev g, T theta, const T* __restrict__ u, const T* __restrict__ sbar, T* __restrict__ gb,
                                                      double* __restrict__ part) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], false);
  double term = 0.0;
  if (in_ip<D>(g, i, j, k)) {
    constexpr int NS = D * (D + 1) / 2;
    T t[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) t[q] = T(0);
    int g0[2] = {0, 0}, g1[2] = {0, 0}, g2[2] = {0, 0};
    const int n0 = 1 + ghost_images(g, 0, i, g0), n1 = 1 + ghost_images(g, 1, j, g1), n2 = D == 3 ? 1 + ghost_images(g, 2, k, g2) : 1;
#pragma unroll 1
    for (int q2 = 0; q2 < n2; ++q2)
#pragma unroll 1
      for (int q1 = 0; q1 < n1; ++q1)
#pragma unroll 1
        for (int q0 = 0; q0 < n0; ++q0) {
          const int J[3] = {q0 == 0 ? i : (q0 == 1 ? g0[0] : g0[1]), q1 == 0 ? j : (q1 == 1 ? g1[0] : g1[1]), q2 == 0 ? k : (q2 == 1 ? g2[0] : g2[1])};
          sigbar_at<D, T>(g, sbar, J, t);
        }
    Mat<D, T> S;
    if constexpr (UNI) {
      strain_uniform<D, T>(g, u, c, I, S);
    } else {
      Mat<D, T> R;
      strain_rotation<D, T>(g, u, c, I, S, R);
    }
    T d2 = T(0);
#pragma unroll
    for (int a = 0; a < D; ++a) d2 += (T)g.dx[a][I[a]] * (T)g.dx[a][I[a]];
    T ms = T(0);  // M:S = Σ_{a<=b} σ̄_ab S_ab
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = a; b < D; ++b) ms += t[sym_index<D>(a, b)] * S.m[a][b];
    const T mag = sqrt(2 * mdot<D, T>(S, S));
    const bool live = mag > T(0);
    const T c2 = 2 * theta * theta * d2;
    const T k1 = c2 * mag, k2 = live ? c2 * 2 * ms / mag : T(0);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        const T m = (a == b ? T(1) : T(0.5)) * t[sym_index<D>(a, b)];
        gb[(long long)(a * D + b) * g.sc + c] = live ? k1 * m + k2 * S.m[a][b] : T(0);
      }
    term = (double)(2 * d2 * mag * ms);
  }
  if (part) {  // kernel argument: uniform over the workgroup
    __shared__ double lds[256];
    const int tid = threadIdx.y * 64 + threadIdx.x;
    lds[tid] = term;
    __syncthreads();
#pragma unroll
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) lds[tid] += lds[tid + h];
      __syncthreads();
    }
    if (tid == 0) part[(blockIdx.z * gridDim.y + blockIdx.y) * (long long)gridDim.x + blockIdx.x] = lds[0];
  }
}

// tail: *thetabar += 2θ Σ_q part[q].  One workgroup; work-item t sums the partials t·m .. (t+1)·m - 1 in index order, then work-item 0 sums the
// 256 segment sums in index order: the same additions in the same order on every run.
static __global__ __launch_bounds__(256) void k_smag_thetabar(long long n, const double* __restrict__ part, double theta, double* __restrict__ thetabar) {
  __shared__ double lds[256];
  const long long m = (n + 255) / 256;
  const long long lo = threadIdx.x * m, hi = lo + m < n ? lo + m : n;
  double v = 0.0;
  for (long long q = lo; q < hi; ++q) v += part[q];
  lds[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double sum = 0.0;
    for (int q = 0; q < 256; ++q) sum += lds[q];
    *thetabar += 2.0 * theta * sum;
  }
}

// number of workgroups of pass 1 = number of partials
inline long long smag_partials(const Launch3& l) { return (long long)l.grid.x * l.grid.y * l.grid.z; }

// pass 1 and the tail on stream s; gb: the ∇ubar scratch as T; part: the grid handle's partials (used only when thetabar != nullptr)
template <typename T>
int launch_smag_gradbar(const ins_grid* G, T theta, const T* u, const T* sbar, T* gb, double* part, double* thetabar, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  double* p = thetabar ? part : nullptr;
  if (G->uniform_exact)
    INS_LAUNCH_D((k_smag_gradbar<D, T, true>), l, s, g, theta, u, sbar, gb, p);
  else
    INS_LAUNCH_D((k_smag_gradbar<D, T, false>), l, s, g, theta, u, sbar, gb, p);
  if (thetabar) {
    hipLaunchKernelGGL(k_smag_thetabar, dim3(1), dim3(256), 0, s, smag_partials(l), part, (double)theta, thetabar);
    INS_LAUNCH_CHECK();
  }
  return INS_OK;
}

}  // namespace
