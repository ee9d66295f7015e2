// Reverse-mode pullbacks of the step operators in fp64 (operators.jl:100-616, boundary_conditions.jl:114-230, 290-516,
// pressure.jl:15-19): each is the exact transpose of THIS library's forward operator on the whole padded array,
// ghost volumes included (DESIGN.md "Differentiability").
//
// The generic gather kernels are the templates of ins_adjoint_kernels.h with T = double (ins_adjoint32.hip instantiates the same
// templates with float); the metric tables and reciprocal conventions are those of the generic forward twins in ins_operators.hip.
// This file adds what is fp64 only: the tiled momentum pullback of uniform periodic 3-D boxes, and the entry points.
#include "ins_adjoint_kernels.h"
#include "ins_wave64.h"

namespace {

// --------------------------------------------------------------------------------------------
// Tiled fused momentum pullback: uniform, all-periodic 3-D boxes (the k_flux64 idioms)
//   x along the 64-lane wavefront, 62 output columns per wavefront (lanes 0 and 63 carry the x halos; x neighbours by DPP shifts), one
//   padded row per wavefront, and a register march in z: each lane holds u and φ for rows y-1..y+1 on planes z-1..z+1 and loads one new
//   plane per step.  Workgroups are ordered so the 8 XCDs each take a contiguous band of rows (as k_flux64).
//   On such a box every interior volume is a DOF of every component, so with φ masked to the interior and everything outside the
//   padded array read as 0, the terms of k_convdiff_adjoint become branch-free: ψαβ(f) = rαβ (φmα[f+eβ] − φmα[f]), and a flux whose
//   ψ vanishes contributes 0 whatever u it reads.  Same sums as the generic kernel with the metric tables taken as constants
//   (G->uniform_exact: constant to 4·N·eps), so the two agree to rounding.
// --------------------------------------------------------------------------------------------
struct AdjTiledArgs {
  int N0, N1, N2;
  int ntx, nty, nzc, zc;
  long long sy, sz, sc;
  double r[3][3];     // r[α][β]: 1/Δuβ (α == β) or 1/Δβ
  double dco[3][3];   // ν · r[γ][β] · (mdx | mdxu)β: diffusion coefficient
  double a1[3][3], a2[3][3];  // [β][α]: A₁βα, A₂βα
  const double* u;
  const double* phi;
  double* ubar;
};

constexpr int ADJ_NW = 4;   // wavefronts (rows) per workgroup
constexpr int ADJ_ZC = 32;  // planes per workgroup

// Component q at this lane's volume + (dx, dy, dz), |d| <= 1: y / z from the register window, x by a DPP shift (all lanes active).
// Called with indices that are constants after unrolling, so the window stays in registers.
__device__ __forceinline__ double at(const double (&W)[3][3][3], int q, int dx, int dy, int dz) {
  const double v = W[q][dy + 1][dz + 1];
  return dx == 1 ? next_h(v, 0.0) : dx == -1 ? prev_h(v, 0.0) : v;
}

// The cotangent at linear index idx of the vector field: a.phi[idx], or, with one more kernel argument, the combination of ins_adjoint_kernels.h
// (PhiComb) formed at this one load site.
template <typename... PC>
__device__ __forceinline__ double tiled_phi(const AdjTiledArgs& a, long long idx, const PC&... pc) {
  if constexpr (sizeof...(PC) == 0)
    return a.phi[idx];
  else
    return (PhiCombAt<double, INS_ADJ_COMB_MAX>{pc, 0}[idx], ...);
}

template <bool ACC, typename... PC>
__global__ __launch_bounds__(64 * ADJ_NW) void k_momentum_pullback_tiled(AdjTiledArgs a, PC... pc) {
  const int nty_local = (a.nty + 7) >> 3;
  int seq = (int)(blockIdx.x >> 3);
  if (seq >= a.ntx * nty_local * a.nzc) return;
  const int txi = seq % a.ntx;
  seq /= a.ntx;
  const int tyi = (int)(blockIdx.x & 7) * nty_local + seq % nty_local;
  const int tzi = seq / nty_local;
  if (tyi >= a.nty) return;
  const int lane = threadIdx.x;
  const int y = tyi * ADJ_NW + __builtin_amdgcn_readfirstlane(threadIdx.y);
  if (y >= a.N1) return;  // whole wavefront
  const int P = txi * 62 + lane - 1;  // padded column of this lane
  const bool colin = P >= 0 && P < a.N0;
  const bool colint = P >= 1 && P <= a.N0 - 2;
  const int k0 = tzi * a.zc, k1 = min(k0 + a.zc, a.N2);

  double U[3][3][3], F[3][3][3];  // [component][dy + 1][dz + 1] at this lane's column
  auto load_plane = [&](int slot, int kz) {
    const bool zin = kz >= 0 && kz < a.N2, zint = kz >= 1 && kz <= a.N2 - 2;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int yy = y + dy - 1;
      const bool ok = colin && zin && yy >= 0 && yy < a.N1;
      const bool okp = colint && zint && yy >= 1 && yy <= a.N1 - 2;
      const long long c = P + yy * a.sy + kz * a.sz;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        U[q][dy][slot] = ok ? a.u[q * a.sc + c] : 0.0;
        F[q][dy][slot] = okp ? tiled_phi(a, q * a.sc + c, pc...) : 0.0;
      }
    }
  };
  load_plane(0, k0 - 1);
  load_plane(1, k0);
  for (int k = k0; k < k1; ++k) {
    load_plane(2, k + 1);
    double out[3];
#pragma unroll
    for (int ga = 0; ga < 3; ++ga) {
      const int g0 = ga == 0, g1 = ga == 1, g2 = ga == 2;  // e_γ
      double v = 0.0;
#pragma unroll
      for (int be = 0; be < 3; ++be) {
        const int b0 = be == 0, b1 = be == 1, b2 = be == 2;  // e_β
        const double f0 = at(F, ga, 0, 0, 0);
        // diffusion
        v += a.dco[ga][be] * (at(F, ga, b0, b1, b2) + at(F, ga, -b0, -b1, -b2) - 2.0 * f0);
        // (a) α = γ, direction β
        const double rg = a.r[ga][be];
        const double p0 = rg * (at(F, ga, b0, b1, b2) - f0);
        const double p1 = rg * (f0 - at(F, ga, -b0, -b1, -b2));
        v += 0.5 * (p0 * (a.a2[be][ga] * at(U, be, 0, 0, 0) + a.a1[be][ga] * at(U, be, g0, g1, g2)) +
                    p1 * (a.a2[be][ga] * at(U, be, -b0, -b1, -b2) + a.a1[be][ga] * at(U, be, g0 - b0, g1 - b1, g2 - b2)));
        // (b) β = γ, component α = be
        const int al = be;
        const double fa = at(F, al, 0, 0, 0);
        const double ra = a.r[al][ga];
        const double q0 = ra * (at(F, al, g0, g1, g2) - fa);
        const double q1 = ra * (at(F, al, g0 - b0, g1 - b1, g2 - b2) - at(F, al, -b0, -b1, -b2));
        v += 0.5 * (q0 * (at(U, al, 0, 0, 0) + at(U, al, g0, g1, g2)) * a.a2[ga][al] +
                    q1 * (at(U, al, -b0, -b1, -b2) + at(U, al, g0 - b0, g1 - b1, g2 - b2)) * a.a1[ga][al]);
      }
      out[ga] = v;
    }
    if (lane >= 1 && lane <= 62 && colin) {
      const long long c = P + y * a.sy + k * a.sz;
#pragma unroll
      for (int ga = 0; ga < 3; ++ga) {
        double* o = a.ubar + ga * a.sc + c;
        *o = ACC ? *o + out[ga] : out[ga];
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        U[q][dy][0] = U[q][dy][1];
        U[q][dy][1] = U[q][dy][2];
        F[q][dy][0] = F[q][dy][1];
        F[q][dy][1] = F[q][dy][2];
      }
  }
}


template <int MODE, bool ACC>
int launch_convdiff_adjoint(const ins_grid* G, double visc, const double* u, const double* phi, double* ubar, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  INS_LAUNCH_D((k_convdiff_adjoint<D, double, MODE, ACC>), l, s, g, visc, u, phi, ubar);
  return INS_OK;
}


bool adj_tiled_supported(const ins_grid* G) {
  return G->g.D == 3 && G->all_periodic && G->all_dof && G->uniform_exact && !ins_opt(OPT_INS_DISABLE_ADJ_TILED);
}

int launch_momentum_pullback_tiled(const ins_grid* G, double visc, const double* u, const double* phi, double* ubar, bool acc, hipStream_t s,
                                   const PhiComb<double, INS_ADJ_COMB_MAX>* comb = nullptr) {
  const GridDev& g = G->g;
  const ins_grid_desc_t& d = G->desc;  // host copy of the tables
  AdjTiledArgs a;
  a.N0 = g.N[0];
  a.N1 = g.N[1];
  a.N2 = g.N[2];
  a.sy = g.sx[1];
  a.sz = g.sx[2];
  a.sc = g.sc;
  for (int al = 0; al < 3; ++al)
    for (int be = 0; be < 3; ++be) {
      const double dxb = d.dx[be][1], dxub = d.dxu[be][1];
      a.r[al][be] = al == be ? 1.0 / dxub : 1.0 / dxb;
      const double m = al == be ? (dxb > 2 * INS_EPS ? 1.0 / dxb : 0.0) : (dxub > 2 * INS_EPS ? 1.0 / dxub : 0.0);
      a.dco[al][be] = visc * a.r[al][be] * m;
      a.a1[be][al] = d.A1[be][al][2];
      a.a2[be][al] = d.A2[be][al][1];
    }
  a.u = u;
  a.phi = phi;
  a.ubar = ubar;
  a.ntx = (int)cdiv(a.N0, 62);
  a.nty = (int)cdiv(a.N1, ADJ_NW);
  a.zc = ADJ_ZC;
  a.nzc = (int)cdiv(a.N2, ADJ_ZC);
  const unsigned nb = (unsigned)(8LL * a.ntx * ((a.nty + 7) / 8) * a.nzc);
  if (comb)
    hipLaunchKernelGGL((k_momentum_pullback_tiled<false, PhiComb<double, INS_ADJ_COMB_MAX>>), dim3(nb), dim3(64, ADJ_NW), 0, s, a, *comb);
  else if (acc)
    hipLaunchKernelGGL(k_momentum_pullback_tiled<true>, dim3(nb), dim3(64, ADJ_NW), 0, s, a);
  else
    hipLaunchKernelGGL(k_momentum_pullback_tiled<false>, dim3(nb), dim3(64, ADJ_NW), 0, s, a);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// --------------------------------------------------------------------------------------------
// Member momentum pullback: the 2-D sibling of the tiled kernel above for the members of an ensemble (ins_rk_ensemble.hip), in the idiom of k_flux2d
//   lanes along x, 62 output columns per wavefront (lanes 0 and 63 carry the x halos; x neighbours by DPP shifts), a wavefront marches through the rows
//   of a y-chunk with rows j-1, j, j+1 of both components of u and φ in registers (a 2 x 3 window each, rolled per row: two loads of u and two of φ per
//   output row).  blockIdx.z is the member; its fields lie b·(its stride) elements behind the pointers.  φ is masked to the interior and everything
//   outside the padded array reads as 0, so the terms are the branch-free ones of the 3-D kernel with the z direction dropped: the same sums as
//   k_convdiff_adjoint<2, double, 3, ·> with the metric tables taken as constants.  The whole padded array of ubar is written (ghost volumes too).
//   Chunking and tile walk depend on the grid only, so member b is bitwise what one member alone gives.
// --------------------------------------------------------------------------------------------
struct Adj2dArgs {
  int N0, N1;
  int yc;  // rows per chunk
  long long sc;
  double r[2][2];              // r[α][β]: 1/Δuβ (α == β) or 1/Δβ
  double dco[2][2];            // ν · r[γ][β] · (mdx | mdxu)β: diffusion coefficient
  double a1[2][2], a2[2][2];   // [β][α]: A₁βα, A₂βα
  const double* u;
  const double* phi;
  double* ubar;
};

// Component q at this lane's volume + (dx, dy), |d| <= 1: y from the register window, x by a DPP shift (all lanes active); constant indices after unrolling.
__device__ __forceinline__ double at2(const double (&W)[2][3], int q, int dx, int dy) {
  const double v = W[q][dy + 1];
  return dx == 1 ? next_h(v, 0.0) : dx == -1 ? prev_h(v, 0.0) : v;
}

template <bool ACC>
__global__ __launch_bounds__(256) void k_momentum_pullback_members_2d(Adj2dArgs a, long long ustride, long long pstride, long long bstride) {
  const long long b = blockIdx.z;
  const int lane = threadIdx.x;
  const int j0 = ((int)blockIdx.y * 4 + __builtin_amdgcn_readfirstlane(threadIdx.y)) * a.yc;  // first output row (padded index)
  if (j0 >= a.N1) return;  // whole wavefront
  const int j1 = min(j0 + a.yc, a.N1);
  const int P = (int)blockIdx.x * 62 + lane - 1;  // padded column of this lane
  const bool colin = P >= 0 && P < a.N0;
  const bool colint = P >= 1 && P <= a.N0 - 2;
  const double* __restrict__ u = a.u + b * ustride;
  const double* __restrict__ phi = a.phi + b * pstride;
  double* __restrict__ ubar = a.ubar + b * bstride;

  double U[2][3], F[2][3];  // [component][dy + 1] at this lane's column
  auto load_row = [&](int slot, int yy) {
    const bool ok = colin && yy >= 0 && yy < a.N1;
    const bool okp = colint && yy >= 1 && yy <= a.N1 - 2;
    const long long c = P + (long long)yy * a.N0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      U[q][slot] = ok ? u[q * a.sc + c] : 0.0;
      F[q][slot] = okp ? phi[q * a.sc + c] : 0.0;
    }
  };
  load_row(0, j0 - 1);
  load_row(1, j0);
  for (int j = j0; j < j1; ++j) {
    load_row(2, j + 1);
    double out[2];
#pragma unroll
    for (int ga = 0; ga < 2; ++ga) {
      const int g0 = ga == 0, g1 = ga == 1;  // e_γ
      double v = 0.0;
#pragma unroll
      for (int be = 0; be < 2; ++be) {
        const int b0 = be == 0, b1 = be == 1;  // e_β
        const double f0 = at2(F, ga, 0, 0);
        // diffusion
        v += a.dco[ga][be] * (at2(F, ga, b0, b1) + at2(F, ga, -b0, -b1) - 2.0 * f0);
        // (a) α = γ, direction β
        const double rg = a.r[ga][be];
        const double p0 = rg * (at2(F, ga, b0, b1) - f0);
        const double p1 = rg * (f0 - at2(F, ga, -b0, -b1));
        v += 0.5 * (p0 * (a.a2[be][ga] * at2(U, be, 0, 0) + a.a1[be][ga] * at2(U, be, g0, g1)) +
                    p1 * (a.a2[be][ga] * at2(U, be, -b0, -b1) + a.a1[be][ga] * at2(U, be, g0 - b0, g1 - b1)));
        // (b) β = γ, component α = be
        const int al = be;
        const double fa = at2(F, al, 0, 0);
        const double ra = a.r[al][ga];
        const double q0 = ra * (at2(F, al, g0, g1) - fa);
        const double q1 = ra * (at2(F, al, g0 - b0, g1 - b1) - at2(F, al, -b0, -b1));
        v += 0.5 * (q0 * (at2(U, al, 0, 0) + at2(U, al, g0, g1)) * a.a2[ga][al] +
                    q1 * (at2(U, al, -b0, -b1) + at2(U, al, g0 - b0, g1 - b1)) * a.a1[ga][al]);
      }
      out[ga] = v;
    }
    if (lane >= 1 && lane <= 62 && colin) {
      const long long c = P + (long long)j * a.N0;
#pragma unroll
      for (int ga = 0; ga < 2; ++ga) {
        double* o = ubar + ga * a.sc + c;
        *o = ACC ? *o + out[ga] : out[ga];
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      U[q][0] = U[q][1];
      U[q][1] = U[q][2];
      F[q][0] = F[q][1];
      F[q][1] = F[q][2];
    }
  }
}
}  // namespace

// ubar[b] (+)= J_F(u[b])ᵀ phi[b] for the nb members of an ensemble in one launch (blockIdx.z = member); the grid is one of the chained 2-D loop (all-periodic,
// every volume a DOF, exactly uniform: the caller's predicate).  Coefficients from the host copy of the grid tables, as launch_momentum_pullback_tiled.
int ins_k_momentum_pullback_members_2d(const ins_grid* G, double visc, const double* u, long long ustride, const double* phi, long long pstride, double* ubar,
                                       long long bstride, bool acc, int nb, hipStream_t s) {
  const GridDev& g = G->g;
  const ins_grid_desc_t& d = G->desc;
  if (g.D != 2 || nb < 1 || nb > 65535) {
    ins_set_error("ins_k_momentum_pullback_members_2d: a 2-D grid and 1 .. 65535 members");
    return INS_ERR_INVALID;
  }
  Adj2dArgs a;
  a.N0 = g.N[0];
  a.N1 = g.N[1];
  a.sc = g.sc;
  for (int al = 0; al < 2; ++al)
    for (int be = 0; be < 2; ++be) {
      const double dxb = d.dx[be][1], dxub = d.dxu[be][1];
      a.r[al][be] = al == be ? 1.0 / dxub : 1.0 / dxb;
      const double m = al == be ? (dxb > 2 * INS_EPS ? 1.0 / dxb : 0.0) : (dxub > 2 * INS_EPS ? 1.0 / dxub : 0.0);
      a.dco[al][be] = visc * a.r[al][be] * m;
      a.a1[be][al] = d.A1[be][al][2];
      a.a2[be][al] = d.A2[be][al][1];
    }
  a.u = u;
  a.phi = phi;
  a.ubar = ubar;
  // rows per chunk as the forward stage kernel chooses them (ins_flux2d.hip): a function of the grid only
  const int ntx = (int)cdiv(a.N0, 62);
  const int want_chunks = std::max(1, 2048 / ntx);
  a.yc = std::min(64, std::max(4, a.N1 / want_chunks));
  const dim3 grid(ntx, cdiv(cdiv(a.N1, a.yc), 4), (unsigned)nb), block(64, 4, 1);
  if (acc)
    hipLaunchKernelGGL(k_momentum_pullback_members_2d<true>, grid, block, 0, s, a, ustride, pstride, bstride);
  else
    hipLaunchKernelGGL(k_momentum_pullback_members_2d<false>, grid, block, 0, s, a, ustride, pstride, bstride);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------
// internal launchers
// ------------------------------------------------------------------------------------------------
static int ins_k_divergence_adjoint(const ins_grid* G, const double* phi, double* ubar, double alpha, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  INS_LAUNCH_D((k_divergence_adjoint<D, double, double>), l, s, g, phi, ubar, alpha);
  return INS_OK;
}

static int ins_k_pressuregradient_adjoint(const ins_grid* G, const double* phi, double* pbar, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  INS_LAUNCH_D((k_pressuregradient_adjoint<D, double, double, true>), l, s, g, phi, pbar);
  return INS_OK;
}

int ins_k_apply_bc_u_pullback(const ins_grid* G, double* u, hipStream_t s) {
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k_apply_bc_u
    if (g.bc[be][0] == INS_BC_HALO && g.bc[be][1] == INS_BC_HALO) continue;
    INS_LAUNCH_D((k_bc_u_pullback<D, double>), line_launch(g, be, g.D), s, g, u, be);
  }
  return INS_OK;
}

int ins_k_apply_bc_p_pullback(const ins_grid* G, double* p, hipStream_t s) {
  const GridDev& g = G->g;
  for (int be = g.D - 1; be >= 0; --be) {  // reverse of ins_k_apply_bc_p_fields
    const int l = g.bc[be][0], r = g.bc[be][1];
    if ((l == INS_BC_DIRICHLET || l == INS_BC_HALO) && (r == INS_BC_DIRICHLET || r == INS_BC_HALO)) continue;
    INS_LAUNCH_D((k_bc_p_pullback<D, double>), line_launch(g, be, 1), s, g, p, be);
  }
  return INS_OK;
}

// ubar = J(u)ᵀ (Σ_q coefs[q]·ks[q]), 1 <= nterms <= INS_ADJ_COMB_MAX: the momentum pullback with the cotangent combined where it is loaded
// (the reverse Runge-Kutta stage, ins_rk_adjoint.hip).  Same dispatch as ins_momentum_pullback_f64.
int ins_k_momentum_pullback_comb(const ins_grid* G, double visc, const double* u, int nterms, const double* coefs, const double* const* ks, double* ubar,
                                 hipStream_t s) {
  INS_REQUIRE(nterms >= 1 && nterms <= INS_ADJ_COMB_MAX, "bad number of cotangent terms");
  PhiComb<double, INS_ADJ_COMB_MAX> pc;
  pc.n = nterms;
  for (int q = 0; q < INS_ADJ_COMB_MAX; ++q) {
    pc.p[q] = q < nterms ? ks[q] : nullptr;
    pc.w[q] = q < nterms ? coefs[q] : 0.0;
  }
  if (adj_tiled_supported(G)) return launch_momentum_pullback_tiled(G, visc, u, nullptr, ubar, false, s, &pc);
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  INS_LAUNCH_D((k_convdiff_adjoint<D, double, 3, false, PhiComb<double, INS_ADJ_COMB_MAX>>), l, s, g, visc, u, pc, ubar);
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_divergence_adjoint_f64(const ins_grid_t* G, const double* phi, double* ubar, void* stream) {
  INS_REQUIRE(G && phi && ubar, "null argument");
  return ins_k_divergence_adjoint(G, phi, ubar, 1.0, as_stream(stream));
}

extern "C" int ins_pressuregradient_adjoint_f64(const ins_grid_t* G, const double* phi, double* pbar, void* stream) {
  INS_REQUIRE(G && phi && pbar, "null argument");
  return ins_k_pressuregradient_adjoint(G, phi, pbar, as_stream(stream));
}

extern "C" int ins_convection_adjoint_f64(const ins_grid_t* G, const double* u, const double* phibar, double* ubar, void* stream) {
  INS_REQUIRE(G && u && phibar && ubar, "null argument");
  INS_REQUIRE(ubar != u && ubar != phibar, "convection_adjoint! cannot run in place");
  return launch_convdiff_adjoint<1, true>(G, 0.0, u, phibar, ubar, as_stream(stream));
}

extern "C" int ins_diffusion_adjoint_f64(const ins_grid_t* G, double visc, const double* phibar, double* ubar, void* stream) {
  INS_REQUIRE(G && phibar && ubar, "null argument");
  INS_REQUIRE(ubar != phibar, "diffusion_adjoint! cannot run in place");
  return launch_convdiff_adjoint<2, true>(G, visc, nullptr, phibar, ubar, as_stream(stream));
}

extern "C" int ins_momentum_pullback_f64(const ins_grid_t* G, double visc, const double* u, const double* phibar, double* ubar, int accumulate,
                                         void* stream) {
  INS_REQUIRE(G && u && phibar && ubar, "null argument");
  INS_REQUIRE(ubar != u && ubar != phibar, "momentum pullback cannot run in place");
  if (adj_tiled_supported(G)) return launch_momentum_pullback_tiled(G, visc, u, phibar, ubar, accumulate != 0, as_stream(stream));
  if (accumulate) return launch_convdiff_adjoint<3, true>(G, visc, u, phibar, ubar, as_stream(stream));
  return launch_convdiff_adjoint<3, false>(G, visc, u, phibar, ubar, as_stream(stream));
}

extern "C" int ins_apply_bc_u_pullback_f64(const ins_grid_t* G, double* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  return ins_k_apply_bc_u_pullback(G, phibar, as_stream(stream));
}

extern "C" int ins_apply_bc_p_pullback_f64(const ins_grid_t* G, double* phibar, void* stream) {
  INS_REQUIRE(G && phibar, "null argument");
  return ins_k_apply_bc_p_pullback(G, phibar, as_stream(stream));
}

// project(u) = u − G·bc_p(poisson(Ω·(D·u)))  =>  φ ← φ − Dᵀ·Ω·poisson·bc_pᵀ·Gᵀ·φ   (the solve is symmetric on the padded arrays).
// All launches on one stream; `pwork` is a scalar field of scratch.
extern "C" int ins_project_pullback_f64(const ins_grid_t* G, ins_poisson_t* ps, double* phibar, double* pwork, void* stream) {
  INS_REQUIRE(G && ps && phibar && pwork, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  INS_REQUIRE(phibar != pwork, "pwork must be its own array");
  hipStream_t s = as_stream(stream);
  int rc;
  INS_HIP_TRY(hipMemsetAsync(pwork, 0, G->ncell * sizeof(double), s));
  if ((rc = ins_k_pressuregradient_adjoint(G, phibar, pwork, s))) return rc;
  if ((rc = ins_k_apply_bc_p_pullback(G, pwork, s))) return rc;
  if ((rc = ins_k_poisson_solve(ps, pwork, s))) return rc;
  if ((rc = ins_k_scalewithvolume(G, pwork, s))) return rc;
  return ins_k_divergence_adjoint(G, pwork, phibar, -1.0, s);
}
