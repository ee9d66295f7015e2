// Differentiable tensor-basis closure (tensorbasis.jl:1-95, operators.jl:1023-1033, 1155-1287; Silvis et al. eqs. 9 and 11):
//   τ = Σ_i a_i B_i(S, R),   V = invariants of (S, R),   S, R = sym / skew of ∇u at a pressure point,
// with all eleven tensors formed in registers from the D·D entries of ∇u: no B field is ever stored
// (k_tensorbasis, ins_fields.hip, writes 11·9 + 5 doubles per cell).  fp64, 2-D and 3-D, stretched grids, any BC mix.
//
// Pullbacks are exact transposes on the whole padded array, masked to the forward's write set Ip, and free of
// atomic operations: pass 1, one work-item per pressure point, forms ∇ubar (D·D doubles) from S, R, the cotangents and a;
// pass 2, one work-item per u entry, gathers the transpose of ∇ from the neighbouring ∇ubar.  Every output is written once by one
// work-item in a fixed order of additions, so results are bitwise reproducible run to run.  The ∇ubar scratch belongs to the grid
// handle (grown on first use).
//
// The matrix helpers, strain_rotation, the basis tensors, the invariants and the reverse rules are in ins_tensorbasis.h, shared with the
// Float32 kernels (ins_tensorclosure32.hip).
#include "ins_tensorbasis.h"

namespace {

// --------------------------------------------------------------------------------------------
// forward: invariants and fused stress (write Ip)
// --------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void k_tc_invariants(GridDev g, const double* __restrict__ u, double* __restrict__ V) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D> S, R;
  strain_rotation<D>(g, u, c, I, S, R);
  double v[5];
  invariants<D>(S, R, v);
  constexpr int nv = D == 2 ? 2 : 5;
#pragma unroll
  for (int q = 0; q < nv; ++q) V[q * g.sc + c] = v[q];
}

template <int D>
__global__ __launch_bounds__(256) void k_tc_stress(GridDev g, const double* __restrict__ u, const double* __restrict__ a, double* __restrict__ tau) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D> S, R;
  strain_rotation<D>(g, u, c, I, S, R);
  Mat<D> T = mzero<D>();
  for_each_basis<D>(S, R, [&](int ib, const Mat<D>& B) { axpy<D>(T, a[ib * g.sc + c], B); });
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int q = p; q < D; ++q) tau[(long long)sym_index<D>(p, q) * g.sc + c] = T.m[p][q];
}

// --------------------------------------------------------------------------------------------
// pass 1 of the pullbacks: ∇ubar at every pressure point
// --------------------------------------------------------------------------------------------
// abar_i = <T, B_i> over the whole padded array (0 outside Ip, where the forward reads no a)
template <int D>
__global__ __launch_bounds__(256) void k_tc_abar(GridDev g, const double* __restrict__ u, const double* __restrict__ taubar, double* __restrict__ abar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  constexpr int nb = D == 2 ? 3 : 11;
  if (!in_ip<D>(g, i, j, k)) {
#pragma unroll
    for (int ib = 0; ib < nb; ++ib) abar[ib * g.sc + c] = 0.0;
    return;
  }
  Mat<D> S, R;
  strain_rotation<D>(g, u, c, I, S, R);
  const Mat<D> T = full_cotangent<D>(g, taubar, c);
  for_each_basis<D>(S, R, [&](int ib, const Mat<D>& B) { abar[ib * g.sc + c] = mdot<D>(T, B); });
}

// closure route: Bbar_i = a_i T, plus the invariants' cotangent
template <int D, bool HASA, bool HASV>
__global__ __launch_bounds__(256) void k_tc_gradbar(GridDev g, const double* __restrict__ u, const double* __restrict__ a, const double* __restrict__ taubar,
                                                    const double* __restrict__ Vbar, double* __restrict__ gb) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D> S, R;
  strain_rotation<D>(g, u, c, I, S, R);
  double vb[5] = {0, 0, 0, 0, 0};
  constexpr int nv = D == 2 ? 2 : 5;
  if (HASV) {
#pragma unroll
    for (int q = 0; q < nv; ++q) vb[q] = Vbar[q * g.sc + c];
  }
  Mat<D> T = mzero<D>();
  if (HASA) T = full_cotangent<D>(g, taubar, c);
  Mat<D> bS, bR;
  basis_reverse<D, double, HASA, HASV>(S, R, [&](int ib) {
    Mat<D> M = T;
    const double s = a[ib * g.sc + c];
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int q = 0; q < D; ++q) M.m[p][q] *= s;
    return M; }, vb, bS, bR);
  put_gradbar<D>(g, gb, c, bS, bR);
}

// operator route: Bbar in the layout of ins_tensorbasis_f64 (element (p, q) of tensor ib at field ib·D·D + p + D·q)
template <int D, bool HASB, bool HASV>
__global__ __launch_bounds__(256) void k_tb_gradbar(GridDev g, const double* __restrict__ u, const double* __restrict__ Bbar, const double* __restrict__ Vbar,
                                                    double* __restrict__ gb) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D> S, R;
  strain_rotation<D>(g, u, c, I, S, R);
  double vb[5] = {0, 0, 0, 0, 0};
  constexpr int nv = D == 2 ? 2 : 5;
  if (HASV) {
#pragma unroll
    for (int q = 0; q < nv; ++q) vb[q] = Vbar[q * g.sc + c];
  }
  Mat<D> bS, bR;
  basis_reverse<D, double, HASB, HASV>(S, R, [&](int ib) {
    Mat<D> M;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int q = 0; q < D; ++q) M.m[p][q] = Bbar[(long long)(ib * D * D + p + D * q) * g.sc + c];
    return M; }, vb, bS, bR);
  put_gradbar<D>(g, gb, c, bS, bR);
}

// --------------------------------------------------------------------------------------------
// pass 2: transpose of ∇ (operators.jl:1023-1033), gathered per u entry over the whole padded array.  ∇ at I reads
//   G_aa(I) = (u_a[I] - u_a[I-e_a]) / Δ_a[I_a]
//   G_ab(I) = ¼ Σ_{d=0,1} [ (u_a[I-d e_a+e_b] - u_a[I-d e_a]) / Δu_b[I_b] + (u_a[I-d e_a] - u_a[I-d e_a-e_b]) / Δu_b[I_b-1] ]
// so u_a[x] collects G_ab-bar at I = x + d e_a + s e_b, s = -1, 0, 1, for I in Ip (the scratch is read nowhere else).
// --------------------------------------------------------------------------------------------
template <int D, bool ACC>
__global__ __launch_bounds__(256) void k_gradu_adjoint(GridDev g, const double* __restrict__ gb, double* __restrict__ ubar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const long long sa = g.sx[a];
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      const double* gab = gb + (long long)(a * D + b) * g.sc;
      if (a == b) {
        if (in_ip<D>(g, i, j, k)) v += gab[c] * g.rdx[a][I[a]];
        int J[3] = {I[0], I[1], I[2]};
        J[a] += 1;
        if (in_ip<D>(g, J[0], J[1], J[2])) v -= gab[c + sa] * g.rdx[a][I[a] + 1];
      } else {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
#pragma unroll
          for (int s = -1; s <= 1; ++s) {
            int J[3] = {I[0], I[1], I[2]};
            J[a] += d;
            J[b] += s;
            if (!in_ip<D>(g, J[0], J[1], J[2])) continue;  // J in Ip: 1 <= J_b <= N_b - 2, both table reads are inside
            const double r1 = g.rdxu[b][J[b]], r0 = g.rdxu[b][J[b] - 1];
            const double w = s < 0 ? r1 : (s == 0 ? r0 - r1 : -r0);
            v += gab[c + d * sa + s * sb] * w / 4;
          }
        }
      }
    }
    double* o = ubar + a * g.sc + c;
    *o = ACC ? *o + v : v;
  }
}

// --------------------------------------------------------------------------------------------
// divoftensor_adjoint (operators.jl:1186-1287): transpose of k_divoftensor on the D(D+1)/2 symmetric fields.  The forward writes, for
// I in Iu[α],  s_α[I] = Σ_β (σ2 - σ1) r_αβ[I_β]  with  σ2 - σ1 = σ_αα[I+e_α] - σ_αα[I]  (α = β, r = 1/Δu)  or
// ¼(σ_αβ[I+e_β] + σ_αβ[I+e_α+e_β] - σ_αβ[I-e_β] - σ_αβ[I+e_α-e_β])  (α ≠ β, r = 1/Δ; the two shared entries cancel).
// An off-diagonal field receives the terms of (α, β) and of (β, α).  Accumulates.
// --------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ double dot_w(const GridDev& g, const double* __restrict__ sbar, int al, int be, const int (&I)[3], int dal, int dbe) {
  int J[3] = {I[0], I[1], I[2]};
  J[al] += dal;
  J[be] += dbe;
  if (!in_iu<D>(g, al, J[0], J[1], J[2])) return 0.0;
  const long long cj = J[0] + J[1] * g.sx[1] + (D == 3 ? J[2] * g.sx[2] : 0);
  return sbar[al * g.sc + cj] * g.rdx[be][J[be]] / 4;
}

template <int D>
__global__ __launch_bounds__(256) void k_divoftensor_adjoint(GridDev g, const double* __restrict__ sbar, double* __restrict__ sigbar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      double v = 0.0;
      if (a == b) {
        int J[3] = {I[0], I[1], I[2]};
        J[a] -= 1;
        if (in_iu<D>(g, a, J[0], J[1], J[2])) v += sbar[a * g.sc + c - g.sx[a]] * g.rdxu[a][J[a]];
        if (in_iu<D>(g, a, i, j, k)) v -= sbar[a * g.sc + c] * g.rdxu[a][I[a]];
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int al = t ? b : a, be = t ? a : b;
          v += dot_w<D>(g, sbar, al, be, I, 0, -1) + dot_w<D>(g, sbar, al, be, I, -1, -1) - dot_w<D>(g, sbar, al, be, I, 0, 1) -
               dot_w<D>(g, sbar, al, be, I, -1, 1);
        }
      }
      sigbar[(long long)sym_index<D>(a, b) * g.sc + c] += v;
    }
}

// the ∇ubar scratch of the grid handle: D·D scalar fields, allocated on first use (all pullbacks of one grid run on one stream at a time)
int gradbar_scratch(const ins_grid* G, double** out) {
  ins_grid* M = const_cast<ins_grid*>(G);
  const size_t need = (size_t)G->g.D * G->g.D * (size_t)G->ncell;
  if (M->gradbar_count < need) {
    if (M->gradbar_dev) INS_HIP_TRY(hipFree(M->gradbar_dev));
    M->gradbar_dev = nullptr;
    M->gradbar_count = 0;
    INS_HIP_TRY(hipMalloc(&M->gradbar_dev, need * sizeof(double)));
    M->gradbar_count = need;
  }
  *out = M->gradbar_dev;
  return INS_OK;
}

int launch_gradu_adjoint(const ins_grid* G, const double* gb, double* ubar, bool acc, hipStream_t s) {
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  if (acc)
    INS_LAUNCH_D((k_gradu_adjoint<D, true>), l, s, g, gb, ubar);
  else
    INS_LAUNCH_D((k_gradu_adjoint<D, false>), l, s, g, gb, ubar);
  return INS_OK;
}

// a z-slab of the multi-GPU decomposition: the pullbacks would have to reduce over the neighbours' ghost planes (not implemented)
bool is_slab(const ins_grid* G) {
  for (int b = 0; b < G->g.D; ++b)
    if (G->g.bc[b][0] == INS_BC_HALO || G->g.bc[b][1] == INS_BC_HALO) return true;
  return false;
}
#define INS_TC_NO_SLAB(G)                                                                    \
  do {                                                                                       \
    if (is_slab(G)) {                                                                        \
      ins_set_error("%s: slab (INS_BC_HALO) grids are not supported", __func__);             \
      return INS_ERR_UNSUPPORTED;                                                            \
    }                                                                                        \
  } while (0)

}  // namespace

// the same scratch for ins_tensorclosure32.hip, which reads the bytes as float
int ins_k_gradbar_scratch(const ins_grid* G, double** out) { return gradbar_scratch(G, out); }

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_tensorinvariants_f64(const ins_grid_t* G, const double* u, double* V, void* stream) {
  INS_REQUIRE(G && u && V, "null argument");
  INS_TC_NO_SLAB(G);
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_tc_invariants<D>), l, as_stream(stream), g, u, V);
  return INS_OK;
}

extern "C" int ins_tensorclosure_stress_f64(const ins_grid_t* G, const double* u, const double* a, double* tau, void* stream) {
  INS_REQUIRE(G && u && a && tau, "null argument");
  INS_TC_NO_SLAB(G);
  INS_REQUIRE(tau != u && tau != a, "tensorclosure stress cannot run in place");
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_tc_stress<D>), l, as_stream(stream), g, u, a, tau);
  return INS_OK;
}

extern "C" int ins_tensorclosure_pullback_f64(const ins_grid_t* G, const double* u, const double* a, const double* taubar, const double* Vbar,
                                              double* abar, double* ubar, int accumulate, void* stream) {
  INS_REQUIRE(G && u && ubar, "null argument");
  INS_TC_NO_SLAB(G);
  INS_REQUIRE((a && taubar && abar) || (!a && !taubar && !abar), "a, taubar and abar are given together or not at all");
  INS_REQUIRE(a || Vbar, "no cotangent: give taubar, Vbar or both");
  INS_REQUIRE(ubar != u && ubar != taubar && ubar != Vbar && ubar != a, "tensorclosure pullback cannot run in place");
  INS_REQUIRE(!abar || (abar != u && abar != taubar && abar != a && abar != Vbar && abar != ubar), "abar must be its own array");
  const GridDev& g = G->g;
  hipStream_t s = as_stream(stream);
  double* gb = nullptr;
  int rc = gradbar_scratch(G, &gb);
  if (rc != INS_OK) return rc;
  if (a) INS_LAUNCH_D((k_tc_abar<D>), box_launch(g.D, g.N), s, g, u, taubar, abar);
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  if (a && Vbar)
    INS_LAUNCH_D((k_tc_gradbar<D, true, true>), l, s, g, u, a, taubar, Vbar, gb);
  else if (a)
    INS_LAUNCH_D((k_tc_gradbar<D, true, false>), l, s, g, u, a, taubar, Vbar, gb);
  else
    INS_LAUNCH_D((k_tc_gradbar<D, false, true>), l, s, g, u, a, taubar, Vbar, gb);
  return launch_gradu_adjoint(G, gb, ubar, accumulate != 0, s);
}

extern "C" int ins_tensorbasis_pullback_f64(const ins_grid_t* G, const double* u, const double* Bbar, const double* Vbar, double* ubar, int accumulate,
                                            void* stream) {
  INS_REQUIRE(G && u && ubar, "null argument");
  INS_TC_NO_SLAB(G);
  INS_REQUIRE(Bbar || Vbar, "no cotangent: give Bbar, Vbar or both");
  INS_REQUIRE(ubar != u && ubar != Bbar && ubar != Vbar, "tensorbasis pullback cannot run in place");
  const GridDev& g = G->g;
  hipStream_t s = as_stream(stream);
  double* gb = nullptr;
  int rc = gradbar_scratch(G, &gb);
  if (rc != INS_OK) return rc;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  if (Bbar && Vbar)
    INS_LAUNCH_D((k_tb_gradbar<D, true, true>), l, s, g, u, Bbar, Vbar, gb);
  else if (Bbar)
    INS_LAUNCH_D((k_tb_gradbar<D, true, false>), l, s, g, u, Bbar, Vbar, gb);
  else
    INS_LAUNCH_D((k_tb_gradbar<D, false, true>), l, s, g, u, Bbar, Vbar, gb);
  return launch_gradu_adjoint(G, gb, ubar, accumulate != 0, s);
}

extern "C" int ins_divoftensor_adjoint_f64(const ins_grid_t* G, const double* sbar, double* sigmabar, void* stream) {
  INS_REQUIRE(G && sbar && sigmabar, "null argument");
  INS_TC_NO_SLAB(G);
  INS_REQUIRE(sbar != sigmabar, "divoftensor_adjoint! cannot run in place");
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.N);
  INS_LAUNCH_D((k_divoftensor_adjoint<D>), l, as_stream(stream), g, sbar, sigmabar);
  return INS_OK;
}
