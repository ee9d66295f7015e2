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
// Reverse rules (derived, not probed).  Every tensor is a sum of products of S and R, evaluated through the binary products
//   SR = S·R, RS = R·S, SS = S·S, RR = R·R, P = SS·RR, Q = RR·SS, ...
// and for Z = X·Y with cotangent Zbar:  Xbar += Zbar·Yᵀ,  Ybar += Xᵀ·Zbar  (the two-factor case of
// X_j bar += (X_1 … X_{j-1})ᵀ Mbar (X_{j+1} … X_k)ᵀ, applied along the product tree);  tr(X·Y) with cotangent v: Xbar += v Yᵀ, Ybar += v Xᵀ.
// S and R are treated as independent full matrices; then ∇ubar = sym(Sbar) + skew(Rbar).
#include "ins_stencil.h"

namespace {

template <int D>
struct Mat {
  double m[D][D];
};

template <int D>
__device__ __forceinline__ Mat<D> mzero() {
  Mat<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) r.m[a][b] = 0.0;
  return r;
}
template <int D>
__device__ __forceinline__ Mat<D> mm(const Mat<D>& x, const Mat<D>& y) {  // x·y, the summation order of mmul in ins_fields.hip
  Mat<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[a][q] * y.m[q][b];
      r.m[a][b] = v;
    }
  return r;
}
template <int D>
__device__ __forceinline__ Mat<D> lin(const Mat<D>& x, const Mat<D>& y, double sy) {  // x + sy·y
  Mat<D> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) r.m[a][b] = x.m[a][b] + sy * y.m[a][b];
  return r;
}
template <int D>
__device__ __forceinline__ void axpy(Mat<D>& z, double s, const Mat<D>& x) {  // z += s·x
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) z.m[a][b] += s * x.m[a][b];
}
template <int D>
__device__ __forceinline__ void axpyT(Mat<D>& z, double s, const Mat<D>& x) {  // z += s·xᵀ
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) z.m[a][b] += s * x.m[b][a];
}
template <int D>
__device__ __forceinline__ void adiag(Mat<D>& z, double s) {  // z += s·I
#pragma unroll
  for (int a = 0; a < D; ++a) z.m[a][a] += s;
}
template <int D>
__device__ __forceinline__ void add_mmt(Mat<D>& z, double s, const Mat<D>& x, const Mat<D>& y) {  // z += s·x·yᵀ
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[a][q] * y.m[b][q];
      z.m[a][b] += s * v;
    }
}
template <int D>
__device__ __forceinline__ void add_mtm(Mat<D>& z, double s, const Mat<D>& x, const Mat<D>& y) {  // z += s·xᵀ·y
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[q][a] * y.m[q][b];
      z.m[a][b] += s * v;
    }
}
template <int D>
__device__ __forceinline__ double mtrace(const Mat<D>& x) {
  double t = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a) t += x.m[a][a];
  return t;
}
template <int D>
__device__ __forceinline__ double mdot(const Mat<D>& x, const Mat<D>& y) {  // Σ x_ab y_ab
  double t = 0.0;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) t += x.m[a][b] * y.m[a][b];
  return t;
}

template <int D>
__host__ __device__ constexpr int sym_index(int a, int b) {  // [xx, yy, (zz), xy, (xz, yz)], as ins_smagtensor_f64
  if (a == b) return a;
  if (D == 2) return 2;
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo == 0 ? (hi == 1 ? 3 : 4) : 5;
}

// ∇(u, I, Δ, Δu) and its symmetric / skew parts at the pressure point I (operators.jl:1023-1033): the expressions of gradu in ins_fields.hip
template <int D>
__device__ __forceinline__ void strain_rotation(const GridDev& g, const double* __restrict__ u, long long c, const int (&I)[3], Mat<D>& S, Mat<D>& R) {
  double G[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const double* ua = u + a * g.sc;
    const long long sa = g.sx[a];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      if (a == b) {
        G[a][b] = (ua[c] - ua[c - sb]) * g.rdx[b][I[b]];
      } else {
        const double r1 = g.rdxu[b][I[b]], r0 = g.rdxu[b][I[b] - 1];
        G[a][b] = ((ua[c + sb] - ua[c]) * r1 + (ua[c - sa + sb] - ua[c - sa]) * r1 + (ua[c] - ua[c - sb]) * r0 +
                   (ua[c - sa] - ua[c - sa - sb]) * r0) /
                  4;
      }
    }
  }
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      S.m[a][b] = (G[a][b] + G[b][a]) / 2;
      R.m[a][b] = (G[a][b] - G[b][a]) / 2;
    }
}

// The basis tensors in the order of tensorbasis.jl:59-69, handed one at a time to f(i, B_i): they live in registers only.
template <int D, class F>
__device__ __forceinline__ void for_each_basis(const Mat<D>& S, const Mat<D>& R, F&& f) {
  Mat<D> Id = mzero<D>();
  adiag<D>(Id, 1.0);
  f(0, Id);
  f(1, S);
  const Mat<D> SR = mm<D>(S, R), RS = mm<D>(R, S);
  f(2, lin<D>(SR, RS, -1.0));
  if constexpr (D == 3) {
    const Mat<D> SS = mm<D>(S, S), RR = mm<D>(R, R);
    f(3, SS);
    f(4, RR);
    f(5, lin<D>(mm<D>(SS, R), mm<D>(R, SS), -1.0));    // S S R - R S S
    f(6, lin<D>(mm<D>(S, RR), mm<D>(RR, S), 1.0));     // S R R + R R S
    f(7, lin<D>(mm<D>(RS, RR), mm<D>(RR, SR), -1.0));  // R S R R - R R S R
    f(8, lin<D>(mm<D>(SR, SS), mm<D>(SS, RS), -1.0));  // S R S S - S S R S
    const Mat<D> P = mm<D>(SS, RR), Q = mm<D>(RR, SS);
    f(9, lin<D>(P, Q, 1.0));                           // S S R R + R R S S
    f(10, lin<D>(mm<D>(R, P), mm<D>(Q, R), -1.0));     // R S S R R - R R S S R
  }
}

// Invariants (tensorbasis.jl:49-50, 70-74), the expressions of k_tensorbasis
template <int D>
__device__ __forceinline__ void invariants(const Mat<D>& S, const Mat<D>& R, double (&V)[5]) {
  if constexpr (D == 2) {
    V[0] = mdot<D>(S, S);
    V[1] = mdot<D>(R, R);
  } else {
    const Mat<D> SS = mm<D>(S, S), RR = mm<D>(R, R);
    V[0] = mtrace<D>(SS);
    V[1] = mtrace<D>(RR);
    V[2] = mtrace<D>(mm<D>(SS, S));
    V[3] = mtrace<D>(mm<D>(S, RR));
    V[4] = mtrace<D>(mm<D>(SS, RR));
  }
}

// Reverse pass at one pressure point: mbar(i) is the cotangent of B_i (i >= 1; B_0 = I is constant), vb that of V.
template <int D, bool HASB, bool HASV, class MB>
__device__ __forceinline__ void basis_reverse(const Mat<D>& S, const Mat<D>& R, MB&& mbar, const double (&vb)[5], Mat<D>& bS, Mat<D>& bR) {
  bS = mzero<D>();
  bR = mzero<D>();
  Mat<D> bSR = mzero<D>(), bRS = mzero<D>();
  if (HASB) {
    axpy<D>(bS, 1.0, mbar(1));  // B1 = S
    const Mat<D> M2 = mbar(2);  // B2 = SR - RS
    axpy<D>(bSR, 1.0, M2);
    axpy<D>(bRS, -1.0, M2);
  }
  if constexpr (D == 2) {
    if (HASV) {  // V0 = Σ S_ab², V1 = Σ R_ab²
      axpy<D>(bS, 2.0 * vb[0], S);
      axpy<D>(bR, 2.0 * vb[1], R);
    }
  } else {
    const Mat<D> SS = mm<D>(S, S), RR = mm<D>(R, R);
    Mat<D> bSS = mzero<D>(), bRR = mzero<D>();
    if (HASB) {
      const Mat<D> SR = mm<D>(S, R), RS = mm<D>(R, S);
      axpy<D>(bSS, 1.0, mbar(3));  // B3 = SS
      axpy<D>(bRR, 1.0, mbar(4));  // B4 = RR
      {                            // B5 = SS·R - R·SS
        const Mat<D> M = mbar(5);
        add_mmt<D>(bSS, 1.0, M, R);
        add_mtm<D>(bR, 1.0, SS, M);
        add_mmt<D>(bR, -1.0, M, SS);
        add_mtm<D>(bSS, -1.0, R, M);
      }
      {  // B6 = S·RR + RR·S
        const Mat<D> M = mbar(6);
        add_mmt<D>(bS, 1.0, M, RR);
        add_mtm<D>(bRR, 1.0, S, M);
        add_mmt<D>(bRR, 1.0, M, S);
        add_mtm<D>(bS, 1.0, RR, M);
      }
      {  // B7 = RS·RR - RR·SR
        const Mat<D> M = mbar(7);
        add_mmt<D>(bRS, 1.0, M, RR);
        add_mtm<D>(bRR, 1.0, RS, M);
        add_mmt<D>(bRR, -1.0, M, SR);
        add_mtm<D>(bSR, -1.0, RR, M);
      }
      {  // B8 = SR·SS - SS·RS
        const Mat<D> M = mbar(8);
        add_mmt<D>(bSR, 1.0, M, SS);
        add_mtm<D>(bSS, 1.0, SR, M);
        add_mmt<D>(bSS, -1.0, M, RS);
        add_mtm<D>(bRS, -1.0, SS, M);
      }
    }
    {  // P = SS·RR, Q = RR·SS:  B9 = P + Q,  B10 = R·P - Q·R,  V4 = tr P
      Mat<D> bP = mzero<D>(), bQ = mzero<D>();
      if (HASB) {
        const Mat<D> M9 = mbar(9);
        axpy<D>(bP, 1.0, M9);
        axpy<D>(bQ, 1.0, M9);
        const Mat<D> M = mbar(10);
        const Mat<D> P = mm<D>(SS, RR), Q = mm<D>(RR, SS);
        add_mmt<D>(bR, 1.0, M, P);
        add_mtm<D>(bP, 1.0, R, M);
        add_mmt<D>(bQ, -1.0, M, R);
        add_mtm<D>(bR, -1.0, Q, M);
      }
      if (HASV) adiag<D>(bP, vb[4]);
      add_mmt<D>(bSS, 1.0, bP, RR);
      add_mtm<D>(bRR, 1.0, SS, bP);
      add_mmt<D>(bRR, 1.0, bQ, SS);
      add_mtm<D>(bSS, 1.0, RR, bQ);
    }
    if (HASV) {
      adiag<D>(bSS, vb[0]);         // V0 = tr SS
      adiag<D>(bRR, vb[1]);         // V1 = tr RR
      axpyT<D>(bSS, vb[2], S);      // V2 = tr(SS·S)
      axpyT<D>(bS, vb[2], SS);
      axpyT<D>(bS, vb[3], RR);      // V3 = tr(S·RR)
      axpyT<D>(bRR, vb[3], S);
    }
    add_mmt<D>(bS, 1.0, bSS, S);  // SS = S·S
    add_mtm<D>(bS, 1.0, S, bSS);
    add_mmt<D>(bR, 1.0, bRR, R);  // RR = R·R
    add_mtm<D>(bR, 1.0, R, bRR);
  }
  add_mmt<D>(bS, 1.0, bSR, R);  // SR = S·R
  add_mtm<D>(bR, 1.0, S, bSR);
  add_mmt<D>(bR, 1.0, bRS, S);  // RS = R·S
  add_mtm<D>(bS, 1.0, R, bRS);
}

// ∇ubar = sym(Sbar) + skew(Rbar) into the scratch: entry (a, b) at field a·D + b
template <int D>
__device__ __forceinline__ void put_gradbar(const GridDev& g, double* __restrict__ gb, long long c, const Mat<D>& bS, const Mat<D>& bR) {
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) gb[(long long)(a * D + b) * g.sc + c] = (bS.m[a][b] + bS.m[b][a]) / 2 + (bR.m[a][b] - bR.m[b][a]) / 2;
}

// The symmetric D×D matrix T with <T, B> = Σ_{a<=b} t_ab B_ab for symmetric B: the cotangent of the D(D+1)/2 stored entries of τ
template <int D>
__device__ __forceinline__ Mat<D> full_cotangent(const GridDev& g, const double* __restrict__ t, long long c) {
  Mat<D> T;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) T.m[a][b] = (a == b ? 1.0 : 0.5) * t[(long long)sym_index<D>(a, b) * g.sc + c];
  return T;
}

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
  basis_reverse<D, HASA, HASV>(S, R, [&](int ib) {
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
  basis_reverse<D, HASB, HASV>(S, R, [&](int ib) {
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
