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
// The fused forward and pass 1 of the pullbacks, with the pointwise part they share, are the templates of ins_tensorbasis.h with T = double
// (ins_tensorclosure32.hip instantiates them with float).  This file holds pass 2 and divoftensor_adjoint (which have float copies in
// ins_tensorclosure32.hip: change both), the ∇ubar scratch, the launches and the fp64 entry points.
#include "ins_tensorbasis.h"

namespace {

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
  if (int rc = M->gradbar_dev.ensure(need)) return rc;
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
#define INS_TC_NO_SLAB(G)                                                                             \
  do {                                                                                                \
    if (int rc_ = no_halo(G, __func__, "slab (INS_BC_HALO) grids are not supported")) return rc_;     \
  } while (0)

}  // namespace

// the same scratch for ins_tensorclosure32.hip, which reads the bytes as float
int ins_k_gradbar_scratch(const ins_grid* G, double** out) { return gradbar_scratch(G, out); }
// pass 2 for ins_smagpullback.hip
int ins_k_gradu_adjoint(const ins_grid* G, const double* gb, double* ubar, bool accumulate, hipStream_t s) { return launch_gradu_adjoint(G, gb, ubar, accumulate, s); }

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_tensorinvariants_f64(const ins_grid_t* G, const double* u, double* V, void* stream) {
  INS_REQUIRE(G && u && V, "null argument");
  INS_TC_NO_SLAB(G);
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_tc_invariants<D, double>), l, as_stream(stream), g, u, V);
  return INS_OK;
}

extern "C" int ins_tensorclosure_stress_f64(const ins_grid_t* G, const double* u, const double* a, double* tau, void* stream) {
  INS_REQUIRE(G && u && a && tau, "null argument");
  INS_TC_NO_SLAB(G);
  INS_REQUIRE(tau != u && tau != a, "tensorclosure stress cannot run in place");
  const GridDev& g = G->g;
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  INS_LAUNCH_D((k_tc_stress<D, double>), l, as_stream(stream), g, u, a, tau);
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
  if (a) INS_LAUNCH_D((k_tc_abar<D, double>), box_launch(g.D, g.N), s, g, u, taubar, abar);
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  if (a && Vbar)
    INS_LAUNCH_D((k_tc_gradbar<D, double, true, true>), l, s, g, u, a, taubar, Vbar, gb);
  else if (a)
    INS_LAUNCH_D((k_tc_gradbar<D, double, true, false>), l, s, g, u, a, taubar, Vbar, gb);
  else
    INS_LAUNCH_D((k_tc_gradbar<D, double, false, true>), l, s, g, u, a, taubar, Vbar, gb);
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
    INS_LAUNCH_D((k_tb_gradbar<D, double, true, true>), l, s, g, u, Bbar, Vbar, gb);
  else if (Bbar)
    INS_LAUNCH_D((k_tb_gradbar<D, double, true, false>), l, s, g, u, Bbar, Vbar, gb);
  else
    INS_LAUNCH_D((k_tb_gradbar<D, double, false, true>), l, s, g, u, Bbar, Vbar, gb);
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
