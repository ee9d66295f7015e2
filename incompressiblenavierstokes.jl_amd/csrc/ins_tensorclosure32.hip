// Differentiable tensor-basis closure with T = Float32 (tensorbasis.jl:1-95, operators.jl:1023-1033, 1155-1287; the reference is generic
// in T):
//   τ = Σ_i a_i B_i(S, R),   V = invariants of (S, R),   s = div τ,   and their pullbacks.
// The fused forward and pass 1 of the pullbacks are the templates of ins_tensorbasis.h with T = float, the ones ins_tensorclosure.hip
// instantiates with double.  Three kernels are still kept here as float copies of their fp64 twins (k32_divoftensor of k_divoftensor in
// ins_fields.hip; k32_gradu_adjoint and k32_divoftensor_adjoint of ins_tensorclosure.hip): the twins spell the shifted index of a mask
// differently, each spelling compiles to a different schedule, and no single one reproduced both.  A fix to one of these
// goes into the other as well.
//
// The conventions of ins_f32g.hip / ins_adjoint32.hip: float fields in the reference layout, the fp64 grid handle, reciprocal tables read
// as doubles and rounded to float where they enter the arithmetic, all arithmetic in float.  The ∇ubar scratch is the grid handle's
// (ins_tensorclosure.hip allocates and grows it, D·D doubles per volume); its first half is used here as D·D floats per volume.  A
// translation unit of its own so that the fp64 kernels keep their register allocation.  Slab (HALO) sides are not taken: the multi-GPU
// path is fp64.
#include "ins_f32_internal.h"
#include "ins_tensorbasis.h"

namespace {

// divoftensor! on the D(D+1)/2 symmetric fields (operators.jl:1203-1236): k_divoftensor of ins_fields.hip in float
template <int D>
__global__ __launch_bounds__(256) void k32_divoftensor(GridDev g, BoxMap L, const float* __restrict__ sig, float* __restrict__ s) {
  INS_BANDED_INDEX(0, 0, 0, g.N[0], g.N[1]);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    if (!in_iu<D>(g, a, i, j, k)) continue;
    const long long sa = g.sx[a];
    float acc = 0.f;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      const float* t = sig + sym_index<D>(a, b) * g.sc;
      float s2, s1;
      if (a == b) {
        s2 = t[c + sb];
        s1 = t[c];
      } else {
        s2 = (t[c] + t[c + sb] + t[c + sa + sb] + t[c + sa]) / 4;
        s1 = (t[c - sb] + t[c] + t[c + sa - sb] + t[c + sa]) / 4;
      }
      acc += (s2 - s1) * (float)(a == b ? g.rdxu[b] : g.rdx[b])[I[b]];
    }
    s[a * g.sc + c] = acc;
  }
}

// --------------------------------------------------------------------------------------------
// pass 2: transpose of ∇, gathered per u entry over the whole padded array (k_gradu_adjoint of ins_tensorclosure.hip, which derives the
// weights): u_a[x] collects G_ab-bar at I = x + d e_a + s e_b, s = -1, 0, 1, for I in Ip (the scratch is read nowhere else).
// --------------------------------------------------------------------------------------------
template <int D, bool ACC>
__global__ __launch_bounds__(256) void k32_gradu_adjoint(GridDev g, const float* __restrict__ gb, float* __restrict__ ubar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const long long sa = g.sx[a];
    float v = 0.f;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      const float* gab = gb + (long long)(a * D + b) * g.sc;
      if (a == b) {
        if (in_ip<D>(g, i, j, k)) v += gab[c] * (float)g.rdx[a][I[a]];
        if (in_ip<D>(g, INS_SH(I, a, 1))) v -= gab[c + sa] * (float)g.rdx[a][I[a] + 1];
      } else {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
#pragma unroll
          for (int s = -1; s <= 1; ++s) {
            int J[3] = {I[0], I[1], I[2]};
            J[a] += d;
            J[b] += s;
            if (!in_ip<D>(g, J[0], J[1], J[2])) continue;  // J in Ip: 1 <= J_b <= N_b - 2, both table reads are inside
            const float r1 = (float)g.rdxu[b][J[b]], r0 = (float)g.rdxu[b][J[b] - 1];
            const float w = s < 0 ? r1 : (s == 0 ? r0 - r1 : -r0);
            v += gab[c + d * sa + s * sb] * w / 4;
          }
        }
      }
    }
    float* o = ubar + a * g.sc + c;
    *o = ACC ? *o + v : v;
  }
}

// --------------------------------------------------------------------------------------------
// divoftensor_adjoint (operators.jl:1186-1287): transpose of k32_divoftensor, k_divoftensor_adjoint of ins_tensorclosure.hip in float.
// An off-diagonal field receives the terms of (α, β) and of (β, α).  Accumulates.
// --------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ float dot_w32(const GridDev& g, const float* __restrict__ sbar, int al, int be, const int (&I)[3], int dal, int dbe) {
  int J[3] = {I[0], I[1], I[2]};
  J[al] += dal;
  J[be] += dbe;
  if (!in_iu<D>(g, al, J[0], J[1], J[2])) return 0.f;
  const long long cj = J[0] + J[1] * g.sx[1] + (D == 3 ? J[2] * g.sx[2] : 0);
  return sbar[al * g.sc + cj] * (float)g.rdx[be][J[be]] / 4;
}

template <int D>
__global__ __launch_bounds__(256) void k32_divoftensor_adjoint(GridDev g, const float* __restrict__ sbar, float* __restrict__ sigbar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) {
      float v = 0.f;
      if (a == b) {
        if (in_iu<D>(g, a, INS_SH(I, a, -1))) v += sbar[a * g.sc + c - g.sx[a]] * (float)g.rdxu[a][I[a] - 1];
        if (in_iu<D>(g, a, i, j, k)) v -= sbar[a * g.sc + c] * (float)g.rdxu[a][I[a]];
      } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int al = t ? b : a, be = t ? a : b;
          v += dot_w32<D>(g, sbar, al, be, I, 0, -1) + dot_w32<D>(g, sbar, al, be, I, -1, -1) - dot_w32<D>(g, sbar, al, be, I, 0, 1) -
               dot_w32<D>(g, sbar, al, be, I, -1, 1);
        }
      }
      sigbar[(long long)sym_index<D>(a, b) * g.sc + c] += v;
    }
}

}  // namespace

// pass 2 for ins_smagpullback32.hip
int ins_k32_gradu_adjoint(const ins_grid* G, const float* gb, float* ubar, bool accumulate, hipStream_t s) {
  const GridDev& g = G->g;
  if (accumulate)
    INS_LAUNCH_D((k32_gradu_adjoint<D, true>), box_launch(g.D, g.N), s, g, gb, ubar);
  else
    INS_LAUNCH_D((k32_gradu_adjoint<D, false>), box_launch(g.D, g.N), s, g, gb, ubar);
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int ins_tensorinvariants_f32(const ins_grid_t* G, const float* u, float* V, void* stream) {
  INS_REQUIRE(G && u && V, "null argument");
  int rc = no_halo(G, "tensorinvariants (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_tc_invariants<D, float>), box_launch(g.D, g.ip_lo, g.ip_hi), as_stream(stream), g, u, V);
  return INS_OK;
}

extern "C" int ins_tensorclosure_stress_f32(const ins_grid_t* G, const float* u, const float* a, float* tau, void* stream) {
  INS_REQUIRE(G && u && a && tau, "null argument");
  int rc = no_halo(G, "tensorclosure stress (f32)");
  if (rc) return rc;
  INS_REQUIRE(tau != u && tau != a, "tensorclosure stress cannot run in place");
  const GridDev& g = G->g;
  INS_LAUNCH_D((k_tc_stress<D, float>), box_launch(g.D, g.ip_lo, g.ip_hi), as_stream(stream), g, u, a, tau);
  return INS_OK;
}

extern "C" int ins_tensorclosure_pullback_f32(const ins_grid_t* G, const float* u, const float* a, const float* taubar, const float* Vbar, float* abar,
                                              float* ubar, int accumulate, void* stream) {
  INS_REQUIRE(G && u && ubar, "null argument");
  int rc = no_halo(G, "tensorclosure pullback (f32)");
  if (rc) return rc;
  INS_REQUIRE((a && taubar && abar) || (!a && !taubar && !abar), "a, taubar and abar are given together or not at all");
  INS_REQUIRE(a || Vbar, "no cotangent: give taubar, Vbar or both");
  INS_REQUIRE(ubar != u && ubar != taubar && ubar != Vbar && ubar != a, "tensorclosure pullback cannot run in place");
  INS_REQUIRE(!abar || (abar != u && abar != taubar && abar != a && abar != Vbar && abar != ubar), "abar must be its own array");
  const GridDev& g = G->g;
  hipStream_t s = as_stream(stream);
  double* gb64 = nullptr;
  if ((rc = ins_k_gradbar_scratch(G, &gb64))) return rc;
  float* gb = reinterpret_cast<float*>(gb64);
  if (a) INS_LAUNCH_D((k_tc_abar<D, float>), box_launch(g.D, g.N), s, g, u, taubar, abar);
  const Launch3 l = box_launch(g.D, g.ip_lo, g.ip_hi);
  if (a && Vbar)
    INS_LAUNCH_D((k_tc_gradbar<D, float, true, true>), l, s, g, u, a, taubar, Vbar, gb);
  else if (a)
    INS_LAUNCH_D((k_tc_gradbar<D, float, true, false>), l, s, g, u, a, taubar, Vbar, gb);
  else
    INS_LAUNCH_D((k_tc_gradbar<D, float, false, true>), l, s, g, u, a, taubar, Vbar, gb);
  if (accumulate)
    INS_LAUNCH_D((k32_gradu_adjoint<D, true>), box_launch(g.D, g.N), s, g, gb, ubar);
  else
    INS_LAUNCH_D((k32_gradu_adjoint<D, false>), box_launch(g.D, g.N), s, g, gb, ubar);
  return INS_OK;
}

extern "C" int ins_divoftensor_f32(const ins_grid_t* G, const float* sig, float* s, void* stream) {
  INS_REQUIRE(G && sig && s, "null argument");
  int rc = no_halo(G, "divoftensor (f32)");
  if (rc) return rc;
  const GridDev& g = G->g;
  const Launch3 l = banded_launch(g.D, g.N);
  INS_LAUNCH_D((k32_divoftensor<D>), l, as_stream(stream), g, l.map, sig, s);
  return INS_OK;
}

extern "C" int ins_divoftensor_adjoint_f32(const ins_grid_t* G, const float* sbar, float* sigmabar, void* stream) {
  INS_REQUIRE(G && sbar && sigmabar, "null argument");
  int rc = no_halo(G, "divoftensor_adjoint (f32)");
  if (rc) return rc;
  INS_REQUIRE(sbar != sigmabar, "divoftensor_adjoint! cannot run in place");
  const GridDev& g = G->g;
  INS_LAUNCH_D((k32_divoftensor_adjoint<D>), box_launch(g.D, g.N), as_stream(stream), g, sbar, sigmabar);
  return INS_OK;
}
