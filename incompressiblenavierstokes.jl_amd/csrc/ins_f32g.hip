// The `_f32` family on ANY grid the fp64 family takes (2-D / 3-D; Dirichlet, Symmetric, Pressure and periodic sides; stretched spacings): the reference is
// generic in the element type on every setup (docs/src/manual/precision.md:3-16), not only on the periodic boxes of csrc/ins_f32.hip.
//
//   fields      : Float32 arrays in the reference layout; the grid handle is the fp64 one — metric tables are read as doubles and rounded to float where
//                 they enter the arithmetic (one table for both families; the tables are a few KB and stay in cache);
//   operators   : all arithmetic in float.  The ghost fills and the divergence are the float instantiations of csrc/ins_operator_kernels.h (k_bc_u, k_bc_p,
//                 k_divergence; boundary data constant: no plane buffers).  k32g_momentum and k32g_applypressure stay copies of k_convdiff<D, 3, true>
//                 and k_pressuregradient<D, true> (csrc/ins_operators.hip, which cites the reference lines) — see the note at k32g_momentum;
//   projection  : Ω·div(u) is formed from the float field in DOUBLE, the fp64 solver the caller wrapped (direct = fast diagonalisation, CG, spectral) runs
//                 unchanged, and the pressure is rounded to float once: a mixed-precision projection whose pressure is at least as accurate as a
//                 Float32 factorisation's (the reference's T = Float32 runs its sparse LU in Float32, pressure.jl:101-154).
// Slab (HALO) sides are not taken: the multi-GPU path is fp64.
#include <cmath>

#include "ins_f32_internal.h"
#include "ins_operator_kernels.h"

namespace {

// k32g_momentum / k32g_applypressure (and k32t_diffusion, csrc/ins_temp32.hip) are NOT instantiations of one template shared with k_convdiff /
// k_pressuregradient, and cannot be: under -ffp-contract=on a fused multiply-add forms only inside one expression, and the twins are spelled
// with different statement boundaries.  These form the diffusive difference, ν·(…) − (…) and `u -= ∇p` as FMAs (54 per volume in k32g_momentum<3>); the
// fp64 kernels round d1, d2, the viscous term and the gradient separately (36).  Either spelling, used for both, changes the results of the other
// precision (profiles/forward_generic_isa.md).  So a fix to one of these stencils goes into its twin as well.
//
// momentum! = fill!(F, 0) + convectiondiffusion!                                         operators.jl:647-690, 971
template <int D>
__global__ __launch_bounds__(256) void k32g_momentum(GridDev g, float visc, const float* __restrict__ u, float* __restrict__ F) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  bool inside = true;
#pragma unroll
  for (int a = 0; a < D; ++a) inside = inside && I[a] >= 1 && I[a] <= g.N[a] - 2;
#pragma unroll
  for (int al = 0; al < D; ++al) {
    float* Fa = F + al * g.sc;
    if (!(inside && in_range<D>(I, g.iu_lo[al], g.iu_hi[al]))) {
      Fa[c] = 0.f;
      continue;
    }
    const float* ua = u + al * g.sc;
    const long long sa = g.sx[al];
    const float uc = ua[c];
    float f = 0.f;
#pragma unroll
    for (int be = 0; be < D; ++be) {
      const long long sb = g.sx[be];
      const int ib = I[be], ia = I[al];
      const float um = ua[c - sb], up = ua[c + sb];
      const float r = (float)(al == be ? g.rdxu[be] : g.rdx[be])[ib];
      const float ma = (float)(al == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
      const float mb = (float)(al == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
      const float* ub = u + be * g.sc;
      const double* A1 = g.A1[be][al];
      const double* A2 = g.A2[be][al];
      const float uab1 = (um + uc) * 0.5f, uab2 = (uc + up) * 0.5f;
      const float uba1 = (float)A2[ia - (al == be)] * ub[c - sb] + (float)A1[ia + (al != be)] * ub[c - sb + sa];
      const float uba2 = (float)A2[ia] * ub[c] + (float)A1[ia + 1] * ub[c + sa];
      f += (visc * ((up - uc) * mb - (uc - um) * ma) - (uab2 * uba2 - uab1 * uba1)) * r;
    }
    Fa[c] = f;
  }
}

// applypressure!                                                                          operators.jl:225-233
template <int D>
__global__ __launch_bounds__(256) void k32g_applypressure(GridDev g, float* __restrict__ u, const float* __restrict__ p) {
  INS_VOL_INDEX(g.sx, 1, 1, 1, i > g.N[0] - 2 || j > g.N[1] - 2);
  const float pc = p[c];
#pragma unroll
  for (int a = 0; a < D; ++a)
    if (in_range<D>(I, g.iu_lo[a], g.iu_hi[a])) u[a * g.sc + c] -= (p[c + g.sx[a]] - pc) * (float)g.rdxu[a][I[a]];
}

__global__ __launch_bounds__(256) void k32g_widen(long long n, const float* __restrict__ a, double* __restrict__ b) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) b[t] = (double)a[t];
}
__global__ __launch_bounds__(256) void k32g_round(long long n, const double* __restrict__ a, float* __restrict__ b) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) b[t] = (float)a[t];
}

inline dim3 flat_grid(long long n) { return dim3((unsigned)std::min<long long>((n + 255) / 256, 8192)); }

}  // namespace

int ins_k32g_apply_bc_u(const ins_grid* G, float* u, hipStream_t s, int dudt) {
  const GridDev& g = G->g;
  int rc = no_halo(G, "apply_bc_u (f32)");
  if (rc) return rc;
  for (int be = 0; be < g.D; ++be) {  // direction after direction: edges and corners come out as in the reference (boundary_conditions.jl:162-165)
    INS_LAUNCH_D((k_bc_u<D, float>), line_launch(g, be, g.D), s, g, u, be, dudt, (const float* const*)nullptr);  // constant boundary data
  }
  return INS_OK;
}

// apply_bc_p! on nf scalar fields laid out back to back (field f at p + f·ncell), as ins_k_apply_bc_p_fields: one launch per direction for all of them
int ins_k32g_apply_bc_p_fields(const ins_grid* G, float* p, int nf, hipStream_t s) {
  const GridDev& g = G->g;
  int rc = no_halo(G, "apply_bc_p (f32)");
  if (rc) return rc;
  for (int be = 0; be < g.D; ++be) {
    if (g.bc[be][0] == INS_BC_DIRICHLET && g.bc[be][1] == INS_BC_DIRICHLET) continue;  // no-op (boundary_conditions.jl:388)
    INS_LAUNCH_D((k_bc_p<D, float>), line_launch(g, be, nf), s, g, p, be, nf > 1 ? G->ncell : 0LL);
  }
  return INS_OK;
}
int ins_k32g_apply_bc_p(const ins_grid* G, float* p, hipStream_t s) { return ins_k32g_apply_bc_p_fields(G, p, 1, s); }

int ins_k32g_momentum(const ins_grid* G, float visc, const float* u, float* F, hipStream_t s) {
  const GridDev& g = G->g;
  INS_LAUNCH_D((k32g_momentum<D>), box_launch(g.D, g.N), s, g, visc, u, F);
  return INS_OK;
}

// div[Ip] = divergence(u) (padded float array; volumes outside Ip are left as they are)
int ins_k32g_divergence(const ins_grid* G, const float* u, float* div, hipStream_t s) {
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_divergence<D, float, float, false>), box_launch(g.D, g.ip_lo, g.ip_hi), s, g, u, div);
  return INS_OK;
}

// psolver(p) with a Float32 p around the fp64 solver: widen, solve (pressure.jl:22 on view(p, Ip)), round.  p64: padded fp64 scratch.
int ins_k32g_solve(const ins_grid* G, ins_poisson* ps64, double* p64, float* p, hipStream_t s) {
  hipLaunchKernelGGL(k32g_widen, flat_grid(G->ncell), dim3(256), 0, s, G->ncell, p, p64);
  INS_LAUNCH_CHECK();
  int rc = ins_k_poisson_solve(ps64, p64, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k32g_round, flat_grid(G->ncell), dim3(256), 0, s, G->ncell, p64, p);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// project!(u, setup; psolver, p), T = Float32: divergence! + scalewithvolume! (in double, from the float field), the fp64 solve, p rounded once, apply_bc_p!,
// applypressure! (pressure.jl:69-82).  As in the reference the caller fills the ghost volumes of u before and after.
int ins_k32g_project(const ins_grid* G, ins_poisson* ps64, double* p64, float* u, float* p, hipStream_t s) {
  const GridDev& g = G->g;
  int rc = no_halo(G, "project (f32)");
  if (rc) return rc;
  INS_LAUNCH_D((k_divergence<D, float, double, true>), box_launch(g.D, g.ip_lo, g.ip_hi), s, g, u, p64);
  if ((rc = ins_k_poisson_solve(ps64, p64, s))) return rc;
  hipLaunchKernelGGL(k32g_round, flat_grid(G->ncell), dim3(256), 0, s, G->ncell, p64, p);
  INS_LAUNCH_CHECK();
  if ((rc = ins_k32g_apply_bc_p(G, p, s))) return rc;
  const int lo[3] = {1, 1, 1}, hi[3] = {g.N[0] - 1, g.N[1] - 1, g.N[2] - 1};
  INS_LAUNCH_D((k32g_applypressure<D>), box_launch(g.D, lo, hi), s, g, u, p);
  return INS_OK;
}
