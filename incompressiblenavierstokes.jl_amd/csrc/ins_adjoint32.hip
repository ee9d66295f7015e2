// Reverse-mode pullbacks of the `_f32` family (operators.jl:100-616, boundary_conditions.jl:114-230, 290-516, pressure.jl:15-19, 52-82):
// the Float32 twins of csrc/ins_adjoint.hip, each the exact transpose of the `_f32` forward operator (csrc/ins_f32.hip, ins_f32g.hip) on
// the whole padded array, ghost volumes included (DESIGN.md "Differentiability").
//
// The conventions of ins_f32g.hip: float fields in the reference layout, the fp64 grid handle, metric tables read as doubles and rounded
// to float where they enter the arithmetic, arithmetic in float.  The launch geometry and the in_ip / in_iu / dof masks of ins_adjoint.hip:
// gather form, one work-item per output volume, no atomics, every output written once; 2-D and 3-D, any BC mix, uniform and stretched
// grids.  A translation unit of its own so that the fp64 kernels keep their register allocation (ins_stencil.h).  Slab (HALO) sides are
// not taken: the multi-GPU path is fp64.
#include "ins_stencil.h"

// csrc/ins_f32.hip: the wrapped fp64 solver of a Float32 solver handle (nullptr: a spectral Float32 solver) and its padded fp64 scratch
ins_poisson* ins_k32_wrapped(const ins_poisson32* ps, double** p64);
const ins_grid* ins_k32_solver_grid(const ins_poisson32* ps);
// csrc/ins_adjoint.hip
int ins_k_apply_bc_p_pullback(const ins_grid* G, double* p, hipStream_t s);

namespace {

// --------------------------------------------------------------------------------------------
// divergence_adjoint                                                     operators.jl:127-145
//   ubar[α][I] += alpha · (φ[I]/Δα[Iα] [I ∈ Ip] − φ[I+eα]/Δα[Iα+1] [I+eα ∈ Ip])   over the whole padded array
//   P = float: arithmetic in float.  P = double: φ is the fp64 solver's pressure, the sum is taken in double and rounded once (the mirror
//   of k32g_div<D, double, true>, which forms the solver's right-hand side in double from the float field).
// --------------------------------------------------------------------------------------------
template <int D, typename P>
__global__ __launch_bounds__(256) void k32a_divergence_adjoint(GridDev g, const P* __restrict__ phi, float* __restrict__ ubar, P alpha) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  const bool here = in_ip<D>(g, i, j, k);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    P v = 0;
    if (here) v += phi[c] * (P)g.rdx[a][I[a]];
    if (in_ip<D>(g, INS_SH(I, a, 1))) v -= phi[c + g.sx[a]] * (P)g.rdx[a][I[a] + 1];
    ubar[a * g.sc + c] += (float)(alpha * v);
  }
}

// --------------------------------------------------------------------------------------------
// pressuregradient_adjoint                                               operators.jl:180-199
//   pbar[I] += Σα (φα[I−eα]/Δuα[Iα−1] [I−eα dof of α] − φα[I]/Δuα[Iα] [I dof of α])
//   P = double, ACC = false: the wrapped solver's fp64 right-hand side Gᵀφ is formed in double from the float cotangent, every volume of
//   the padded array written.
// --------------------------------------------------------------------------------------------
template <int D, typename P, bool ACC>
__global__ __launch_bounds__(256) void k32a_pressuregradient_adjoint(GridDev g, const float* __restrict__ phi, P* __restrict__ pbar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  P v = 0;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float* pa = phi + a * g.sc;
    if (dof<D>(g, a, i, j, k)) v -= (P)pa[c] * (P)g.rdxu[a][I[a]];
    if (dof<D>(g, a, INS_SH(I, a, -1))) v += (P)pa[c - g.sx[a]] * (P)g.rdxu[a][I[a] - 1];
  }
  pbar[c] = ACC ? pbar[c] + v : v;
}

// --------------------------------------------------------------------------------------------
// momentum pullback                                             operators.jl:417-519, 575-616
//   k_convdiff_adjoint<D, 3, ACC> (ins_adjoint.hip, which derives the terms) in float: the transpose of k32g_momentum's Jacobian at u.
//   A flux is evaluated only where ψ has a DOF term, i.e. exactly where the forward evaluated it, so every read stays inside the padded
//   array.  ACC: ubar += J^T φ, else ubar = J^T φ.
// --------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ float rr32(const GridDev& g, int al, int be, int ib) {
  return (float)(al == be ? g.rdxu[be] : g.rdx[be])[ib];
}

// ψαβ(f) at f = (f0, f1, f2) (linear index cf); `live` = it has a DOF term
template <int D>
__device__ __forceinline__ float psi32(const GridDev& g, int al, int be, const int (&F)[3], long long cf, const float* __restrict__ phia,
                                       bool& live) {
  const bool d0 = dof<D>(g, al, F[0], F[1], F[2]);
  const bool d1 = dof<D>(g, al, INS_SH(F, be, 1));
  live = d0 || d1;
  float v = 0.f;
  if (d0) v -= rr32<D>(g, al, be, F[be]) * phia[cf];
  if (d1) v += rr32<D>(g, al, be, F[be] + 1) * phia[cf + g.sx[be]];
  return v;
}

template <int D, bool ACC>
__global__ __launch_bounds__(256) void k32a_momentum_pullback(GridDev g, float visc, const float* __restrict__ u, const float* __restrict__ phi,
                                                              float* __restrict__ ubar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);

#pragma unroll
  for (int ga = 0; ga < D; ++ga) {
    const float* pg = phi + ga * g.sc;
    float v = 0.f;
    {  // diffusion
      const bool dx = dof<D>(g, ga, i, j, k);
#pragma unroll
      for (int be = 0; be < D; ++be) {
        const int ib = I[be];
        const long long sb = g.sx[be];
        // ma(i) = mdx[i] | mdxu[i-1],  mb(i) = mdx[i+1] | mdxu[i]   (k32g_momentum)
        if (dx) {
          const float ma = (float)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
          const float mb = (float)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
          v -= visc * pg[c] * rr32<D>(g, ga, be, ib) * (ma + mb);
        }
        if (dof<D>(g, ga, INS_SH(I, be, -1))) {
          const float mb = (float)(ga == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
          v += visc * pg[c - sb] * rr32<D>(g, ga, be, ib - 1) * mb;
        }
        if (dof<D>(g, ga, INS_SH(I, be, 1))) {
          const float ma = (float)(ga == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
          v += visc * pg[c + sb] * rr32<D>(g, ga, be, ib + 1) * ma;
        }
      }
    }
    const long long sg = g.sx[ga];
    // (a) α = γ: ∂Φγβ(f)/∂uγ = ½ (A₂βγ[fγ] uβ[f] + A₁βγ[fγ+1] uβ[f+eγ])
#pragma unroll
    for (int be = 0; be < D; ++be) {
      const long long sb = g.sx[be];
      const float* ub = u + be * g.sc;
      const double* A1 = g.A1[be][ga];
      const double* A2 = g.A2[be][ga];
#pragma unroll
      for (int sh = 0; sh < 2; ++sh) {  // f = x, x − eβ
        const int F[3] = {INS_SH(I, be, -sh)};
        const long long cf = c - sh * sb;
        bool live;
        const float w = psi32<D>(g, ga, be, F, cf, pg, live);
        if (live) v += w * 0.5f * ((float)A2[F[ga]] * ub[cf] + (float)A1[F[ga] + 1] * ub[cf + sg]);
      }
    }
    // (b) β = γ: ∂Φαγ(f)/∂uγ[f] = ½(uα[f]+uα[f+eγ]) A₂γα[fα];  ∂Φαγ(f)/∂uγ[f+eα] = ½(uα[f]+uα[f+eγ]) A₁γα[fα+1]
#pragma unroll
    for (int al = 0; al < D; ++al) {
      const long long sa = g.sx[al];
      const float* ua = u + al * g.sc;
      const float* pa = phi + al * g.sc;
      const double* A1 = g.A1[ga][al];
      const double* A2 = g.A2[ga][al];
      {
        bool live;
        const float w = psi32<D>(g, al, ga, I, c, pa, live);
        if (live) v += w * 0.5f * (ua[c] + ua[c + sg]) * (float)A2[I[al]];
      }
      {
        const int F[3] = {INS_SH(I, al, -1)};
        const long long cf = c - sa;
        bool live;
        const float w = psi32<D>(g, al, ga, F, cf, pa, live);
        if (live) v += w * 0.5f * (ua[cf] + ua[cf + sg]) * (float)A1[I[al]];
      }
    }
    float* ob = ubar + ga * g.sc + c;
    *ob = ACC ? *ob + v : v;
  }
}

// --------------------------------------------------------------------------------------------
// apply_bc_u_pullback / apply_bc_p_pullback           boundary_conditions.jl:169-230, 290-516
//   The exact transposes of k32g_bc_u / k32g_bc_p (and, on periodic boxes, of k32_bc_periodic, which does the same copies): β = D-1..0
//   and, per line, right side then left side; x[i] = x[j] becomes (x̄[j] += x̄[i]; x̄[i] = 0), x[i] = const becomes x̄[i] = 0.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ void move_to32(float* __restrict__ x, long long from, long long to) {
  const float t = x[from];
  x[from] = 0.f;
  x[to] += t;
}

template <int D>
__global__ __launch_bounds__(256) void k32a_bc_u_pullback(GridDev g, float* __restrict__ u, int be) {
  INS_LINE_INDEX(be);
  const int al = blockIdx.z;
  const long long sb = g.sx[be];
  float* ua = u + al * g.sc + base;
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  if (bcl == INS_BC_PERIODIC) {  // forward: x[ia] = x[ib-1]; x[ib] = x[ia+1]
    const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
    move_to32(ua, ib * sb, (ia + 1) * sb);
    move_to32(ua, ia * sb, (ib - 1) * sb);
    return;
  }
#pragma unroll
  for (int side = 1; side >= 0; --side) {
    const int bc = side ? bcr : bcl;
    const int i = side ? g.iu_hi[al][be] : g.iu_lo[al][be] - 1;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_DIRICHLET || (bc == INS_BC_SYMMETRIC && al == be))
      ua[i * sb] = 0.f;
    else if (bc == INS_BC_SYMMETRIC || bc == INS_BC_PRESSURE)
      move_to32(ua, i * sb, jn * sb);
  }
}

template <int D>
__global__ __launch_bounds__(256) void k32a_bc_p_pullback(GridDev g, float* __restrict__ p, int be) {
  INS_LINE_INDEX(be);
  float* pl = p + base;
  const long long sb = g.sx[be];
  const int bcl = g.bc[be][0], bcr = g.bc[be][1];
  const int ia = g.ip_lo[be] - 1, ib = g.ip_hi[be];
  if (bcl == INS_BC_PERIODIC) {
    move_to32(pl, ib * sb, (ia + 1) * sb);
    move_to32(pl, ia * sb, (ib - 1) * sb);
    return;
  }
#pragma unroll
  for (int side = 1; side >= 0; --side) {
    const int bc = side ? bcr : bcl;
    const int i = side ? ib : ia;
    const int jn = side ? i - 1 : i + 1;
    if (bc == INS_BC_SYMMETRIC)
      move_to32(pl, i * sb, jn * sb);
    else if (bc == INS_BC_PRESSURE)
      pl[i * sb] = 0.f;
  }
}

// Z of the spectral projection pullback: the two ghost planes of direction be of a vector field are set to zero (periodic boxes)
template <int D>
__global__ __launch_bounds__(256) void k32a_zero_ghosts(GridDev g, float* __restrict__ u, int be) {
  INS_LINE_INDEX(be);
  float* ua = u + blockIdx.z * g.sc + base;
  ua[(g.ip_lo[be] - 1) * g.sx[be]] = 0.f;
  ua[g.ip_hi[be] * g.sx[be]] = 0.f;
}

int no_halo(const ins_grid* G, const char* what) {
  for (int a = 0; a < G->g.D; ++a)
    if (G->g.bc[a][0] == INS_BC_HALO || G->g.bc[a][1] == INS_BC_HALO) {
      ins_set_error("%s: slab (halo) grids run in fp64 only", what);
      return INS_ERR_UNSUPPORTED;
    }
  return INS_OK;
}

int bc_u_pullback32(const ins_grid* G, float* u, hipStream_t s) {
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k32g_apply_bc_u
    INS_LAUNCH_D((k32a_bc_u_pullback<D>), line_launch(g, be, g.D), s, g, u, be);
  }
  return INS_OK;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_divergence_adjoint_f32(const ins_grid_t* G, const float* phi, float* ubar, void* stream) {
  INS_REQUIRE(G && phi && ubar, "null argument");
  int rc = no_halo(G, "divergence_adjoint (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  INS_LAUNCH_D((k32a_divergence_adjoint<D, float>), box_launch(g.D, g.N), as_stream(stream), g, phi, ubar, 1.f);
  return INS_OK;
}

extern "C" int ins_pressuregradient_adjoint_f32(const ins_grid_t* G, const float* phi, float* pbar, void* stream) {
  INS_REQUIRE(G && phi && pbar, "null argument");
  int rc = no_halo(G, "pressuregradient_adjoint (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  INS_LAUNCH_D((k32a_pressuregradient_adjoint<D, float, true>), box_launch(g.D, g.N), as_stream(stream), g, phi, pbar);
  return INS_OK;
}

extern "C" int ins_momentum_pullback_f32(const ins_grid_t* G, float visc, const float* u, const float* phibar, float* ubar, int accumulate,
                                         void* stream) {
  INS_REQUIRE(G && u && phibar && ubar, "null argument");
  INS_REQUIRE(ubar != u && ubar != phibar, "momentum pullback cannot run in place");
  int rc = no_halo(G, "momentum pullback (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  if (accumulate)
    INS_LAUNCH_D((k32a_momentum_pullback<D, true>), l, as_stream(stream), g, visc, u, phibar, ubar);
  else
    INS_LAUNCH_D((k32a_momentum_pullback<D, false>), l, as_stream(stream), g, visc, u, phibar, ubar);
  return INS_OK;
}

extern "C" int ins_apply_bc_u_pullback_f32(const ins_grid_t* G, float* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  int rc = no_halo(G, "apply_bc_u pullback (f32)");
  if (rc) return rc;
  return bc_u_pullback32(G, phibar, as_stream(stream));
}

extern "C" int ins_apply_bc_p_pullback_f32(const ins_grid_t* G, float* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  int rc = no_halo(G, "apply_bc_p pullback (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k32g_apply_bc_p
    if (g.bc[be][0] == INS_BC_DIRICHLET && g.bc[be][1] == INS_BC_DIRICHLET) continue;
    INS_LAUNCH_D((k32a_bc_p_pullback<D>), line_launch(g, be, 1), as_stream(stream), g, phibar, be);
  }
  return INS_OK;
}

// Wrapped solver: ins_k32g_project is u ↦ u − G·bc_p(round(poisson(Ω·D u))) on the DOF volumes with D u taken in double from the float field
// (left ghost column included) and every other volume left alone, so φ ← φ − round(Dᵀ·Ω·poisson·bc_pᵀ·Gᵀ·φ) with everything between Gᵀ and
// Dᵀ in double: the order of ins_project_pullback_f64 (Gᵀ, bc_pᵀ, solve, Ω, −Dᵀ) on the solver's fp64 scratch.
// Spectral solver: ins_project_f32 is u ↦ B·P·Z·u on a uniform periodic box (Z: the ghost values are not read, periodic images are; P: the
// projection of the interior; B: the periodic ghost fill of the result).  There G = −Dᵀ and Ω is a constant, so P = I − G·poisson·Ω·D is
// symmetric and the transpose is Z·P·Bᵀ: the ghost-fill pullback, the forward entry itself (the same solver route, so the same accuracy),
// and the ghosts set to zero.
extern "C" int ins_project_pullback_f32(const ins_grid_t* G, ins_poisson32_t* ps, float* phibar, float* pwork, void* stream) {
  INS_REQUIRE(G && ps && phibar && pwork, "null argument");
  INS_REQUIRE(ins_k32_solver_grid(ps) == G, "psolver was created for a different grid");
  INS_REQUIRE(phibar != pwork, "pwork must be its own array");
  int rc = no_halo(G, "project pullback (f32)");
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  const GridDev& g = G->g;
  double* p64 = nullptr;
  ins_poisson* ps64 = ins_k32_wrapped(ps, &p64);
  if (ps64) {
    if (ps64->kind == POISSON_SPECTRAL && G->all_periodic) {
      ins_set_error("project pullback (f32): a wrapped spectral solver on an all-periodic box is not taken (use ins_poisson_spectral_create_f32)");
      return INS_ERR_UNSUPPORTED;
    }
    INS_LAUNCH_D((k32a_pressuregradient_adjoint<D, double, false>), box_launch(g.D, g.N), s, g, phibar, p64);
    if ((rc = ins_k_apply_bc_p_pullback(G, p64, s))) return rc;
    if ((rc = ins_k_poisson_solve(ps64, p64, s))) return rc;
    if ((rc = ins_k_scalewithvolume(G, p64, s))) return rc;
    INS_LAUNCH_D((k32a_divergence_adjoint<D, double>), box_launch(g.D, g.N), s, g, p64, phibar, -1.0);
    // the forward rounds the whole scratch into its p: leave the volumes outside Ip as ins_poisson_wrap_f32 made them
    INS_HIP_TRY(hipMemsetAsync(p64, 0, G->ncell * sizeof(double), s));
    return INS_OK;
  }
  if ((rc = bc_u_pullback32(G, phibar, s))) return rc;
  if ((rc = ins_project_f32(G, ps, phibar, pwork, stream))) return rc;
  for (int be = 0; be < g.D; ++be) {
    INS_LAUNCH_D((k32a_zero_ghosts<D>), line_launch(g, be, g.D), s, g, phibar, be);
  }
  return INS_OK;
}
