// The tensor-basis closure once for both precisions (tensorbasis.jl:1-95, operators.jl:1023-1033; Silvis et al. eqs. 9 and 11), as templates
// over the scalar type T of the fields: ins_tensorclosure.hip instantiates them with double, ins_tensorclosure32.hip with float.
// First the pointwise part: D×D matrices in registers, ∇u and its symmetric / skew parts at a pressure point, the eleven basis tensors, the
// invariants and the reverse rules.  Then the kernels built on it: the fused forward (k_tc_invariants, k_tc_stress) and pass 1 of the
// pullbacks (k_tc_abar, k_tc_gradbar, k_tb_gradbar).  The grid handle is the fp64 one for both: a metric table entry is converted to T where
// it enters, and all arithmetic is in T (ins_adjoint_kernels.h states the rule).
//
// Reverse rules (derived, not probed).  Every tensor is a sum of products of S and R, evaluated through the binary products
//   SR = S·R, RS = R·S, SS = S·S, RR = R·R, P = SS·RR, Q = RR·SS, ...
// and for Z = X·Y with cotangent Zbar:  Xbar += Zbar·Yᵀ,  Ybar += Xᵀ·Zbar  (the two-factor case of
// X_j bar += (X_1 … X_{j-1})ᵀ Mbar (X_{j+1} … X_k)ᵀ, applied along the product tree);  tr(X·Y) with cotangent v: Xbar += v Yᵀ, Ybar += v Xᵀ.
// S and R are treated as independent full matrices; then ∇ubar = sym(Sbar) + skew(Rbar).
#pragma once

#include "ins_stencil.h"

namespace {

template <int D, typename T = double>
struct Mat {
  T m[D][D];
};

template <int D, typename T = double>
__device__ __forceinline__ Mat<D, T> mzero() {
  Mat<D, T> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) r.m[a][b] = T(0);
  return r;
}
template <int D, typename T>
__device__ __forceinline__ Mat<D, T> mm(const Mat<D, T>& x, const Mat<D, T>& y) {  // x·y, the summation order of mmul in ins_fields.hip
  Mat<D, T> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      T v = T(0);
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[a][q] * y.m[q][b];
      r.m[a][b] = v;
    }
  return r;
}
template <int D, typename T>
__device__ __forceinline__ Mat<D, T> lin(const Mat<D, T>& x, const Mat<D, T>& y, T sy) {  // x + sy·y
  Mat<D, T> r;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) r.m[a][b] = x.m[a][b] + sy * y.m[a][b];
  return r;
}
template <int D, typename T>
__device__ __forceinline__ void axpy(Mat<D, T>& z, T s, const Mat<D, T>& x) {  // z += s·x
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) z.m[a][b] += s * x.m[a][b];
}
template <int D, typename T>
__device__ __forceinline__ void axpyT(Mat<D, T>& z, T s, const Mat<D, T>& x) {  // z += s·xᵀ
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) z.m[a][b] += s * x.m[b][a];
}
template <int D, typename T>
__device__ __forceinline__ void adiag(Mat<D, T>& z, T s) {  // z += s·I
#pragma unroll
  for (int a = 0; a < D; ++a) z.m[a][a] += s;
}
template <int D, typename T>
__device__ __forceinline__ void add_mmt(Mat<D, T>& z, T s, const Mat<D, T>& x, const Mat<D, T>& y) {  // z += s·x·yᵀ
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      T v = T(0);
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[a][q] * y.m[b][q];
      z.m[a][b] += s * v;
    }
}
template <int D, typename T>
__device__ __forceinline__ void add_mtm(Mat<D, T>& z, T s, const Mat<D, T>& x, const Mat<D, T>& y) {  // z += s·xᵀ·y
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      T v = T(0);
#pragma unroll
      for (int q = 0; q < D; ++q) v += x.m[q][a] * y.m[q][b];
      z.m[a][b] += s * v;
    }
}
template <int D, typename T>
__device__ __forceinline__ T mtrace(const Mat<D, T>& x) {
  T t = T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) t += x.m[a][a];
  return t;
}
template <int D, typename T>
__device__ __forceinline__ T mdot(const Mat<D, T>& x, const Mat<D, T>& y) {  // Σ x_ab y_ab
  T t = T(0);
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
template <int D, typename T>
__device__ __forceinline__ void strain_rotation(const GridDev& g, const T* __restrict__ u, long long c, const int (&I)[3], Mat<D, T>& S, Mat<D, T>& R) {
  T G[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const T* ua = u + a * g.sc;
    const long long sa = g.sx[a];
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const long long sb = g.sx[b];
      if (a == b) {
        G[a][b] = (ua[c] - ua[c - sb]) * (T)g.rdx[b][I[b]];
      } else {
        const T r1 = (T)g.rdxu[b][I[b]], r0 = (T)g.rdxu[b][I[b] - 1];
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
template <int D, typename T, class F>
__device__ __forceinline__ void for_each_basis(const Mat<D, T>& S, const Mat<D, T>& R, F&& f) {
  Mat<D, T> Id = mzero<D, T>();
  adiag<D, T>(Id, 1.0);
  f(0, Id);
  f(1, S);
  const Mat<D, T> SR = mm<D, T>(S, R), RS = mm<D, T>(R, S);
  f(2, lin<D, T>(SR, RS, -1.0));
  if constexpr (D == 3) {
    const Mat<D, T> SS = mm<D, T>(S, S), RR = mm<D, T>(R, R);
    f(3, SS);
    f(4, RR);
    f(5, lin<D, T>(mm<D, T>(SS, R), mm<D, T>(R, SS), -1.0));    // S S R - R S S
    f(6, lin<D, T>(mm<D, T>(S, RR), mm<D, T>(RR, S), 1.0));     // S R R + R R S
    f(7, lin<D, T>(mm<D, T>(RS, RR), mm<D, T>(RR, SR), -1.0));  // R S R R - R R S R
    f(8, lin<D, T>(mm<D, T>(SR, SS), mm<D, T>(SS, RS), -1.0));  // S R S S - S S R S
    const Mat<D, T> P = mm<D, T>(SS, RR), Q = mm<D, T>(RR, SS);
    f(9, lin<D, T>(P, Q, 1.0));                                 // S S R R + R R S S
    f(10, lin<D, T>(mm<D, T>(R, P), mm<D, T>(Q, R), -1.0));     // R S S R R - R R S S R
  }
}

// Invariants (tensorbasis.jl:49-50, 70-74), the expressions of k_tensorbasis
template <int D, typename T>
__device__ __forceinline__ void invariants(const Mat<D, T>& S, const Mat<D, T>& R, T (&V)[5]) {
  if constexpr (D == 2) {
    V[0] = mdot<D, T>(S, S);
    V[1] = mdot<D, T>(R, R);
  } else {
    const Mat<D, T> SS = mm<D, T>(S, S), RR = mm<D, T>(R, R);
    V[0] = mtrace<D, T>(SS);
    V[1] = mtrace<D, T>(RR);
    V[2] = mtrace<D, T>(mm<D, T>(SS, S));
    V[3] = mtrace<D, T>(mm<D, T>(S, RR));
    V[4] = mtrace<D, T>(mm<D, T>(SS, RR));
  }
}

// Reverse pass at one pressure point: mbar(i) is the cotangent of B_i (i >= 1; B_0 = I is constant), vb that of V.
template <int D, typename T, bool HASB, bool HASV, class MB>
__device__ __forceinline__ void basis_reverse(const Mat<D, T>& S, const Mat<D, T>& R, MB&& mbar, const T (&vb)[5], Mat<D, T>& bS, Mat<D, T>& bR) {
  bS = mzero<D, T>();
  bR = mzero<D, T>();
  Mat<D, T> bSR = mzero<D, T>(), bRS = mzero<D, T>();
  if (HASB) {
    axpy<D, T>(bS, 1.0, mbar(1));  // B1 = S
    const Mat<D, T> M2 = mbar(2);  // B2 = SR - RS
    axpy<D, T>(bSR, 1.0, M2);
    axpy<D, T>(bRS, -1.0, M2);
  }
  if constexpr (D == 2) {
    if (HASV) {  // V0 = Σ S_ab², V1 = Σ R_ab²
      axpy<D, T>(bS, T(2) * vb[0], S);
      axpy<D, T>(bR, T(2) * vb[1], R);
    }
  } else {
    const Mat<D, T> SS = mm<D, T>(S, S), RR = mm<D, T>(R, R);
    Mat<D, T> bSS = mzero<D, T>(), bRR = mzero<D, T>();
    if (HASB) {
      const Mat<D, T> SR = mm<D, T>(S, R), RS = mm<D, T>(R, S);
      axpy<D, T>(bSS, 1.0, mbar(3));  // B3 = SS
      axpy<D, T>(bRR, 1.0, mbar(4));  // B4 = RR
      {                               // B5 = SS·R - R·SS
        const Mat<D, T> M = mbar(5);
        add_mmt<D, T>(bSS, 1.0, M, R);
        add_mtm<D, T>(bR, 1.0, SS, M);
        add_mmt<D, T>(bR, -1.0, M, SS);
        add_mtm<D, T>(bSS, -1.0, R, M);
      }
      {  // B6 = S·RR + RR·S
        const Mat<D, T> M = mbar(6);
        add_mmt<D, T>(bS, 1.0, M, RR);
        add_mtm<D, T>(bRR, 1.0, S, M);
        add_mmt<D, T>(bRR, 1.0, M, S);
        add_mtm<D, T>(bS, 1.0, RR, M);
      }
      {  // B7 = RS·RR - RR·SR
        const Mat<D, T> M = mbar(7);
        add_mmt<D, T>(bRS, 1.0, M, RR);
        add_mtm<D, T>(bRR, 1.0, RS, M);
        add_mmt<D, T>(bRR, -1.0, M, SR);
        add_mtm<D, T>(bSR, -1.0, RR, M);
      }
      {  // B8 = SR·SS - SS·RS
        const Mat<D, T> M = mbar(8);
        add_mmt<D, T>(bSR, 1.0, M, SS);
        add_mtm<D, T>(bSS, 1.0, SR, M);
        add_mmt<D, T>(bSS, -1.0, M, RS);
        add_mtm<D, T>(bRS, -1.0, SS, M);
      }
    }
    {  // P = SS·RR, Q = RR·SS:  B9 = P + Q,  B10 = R·P - Q·R,  V4 = tr P
      Mat<D, T> bP = mzero<D, T>(), bQ = mzero<D, T>();
      if (HASB) {
        const Mat<D, T> M9 = mbar(9);
        axpy<D, T>(bP, 1.0, M9);
        axpy<D, T>(bQ, 1.0, M9);
        const Mat<D, T> M = mbar(10);
        const Mat<D, T> P = mm<D, T>(SS, RR), Q = mm<D, T>(RR, SS);
        add_mmt<D, T>(bR, 1.0, M, P);
        add_mtm<D, T>(bP, 1.0, R, M);
        add_mmt<D, T>(bQ, -1.0, M, R);
        add_mtm<D, T>(bR, -1.0, Q, M);
      }
      if (HASV) adiag<D, T>(bP, vb[4]);
      add_mmt<D, T>(bSS, 1.0, bP, RR);
      add_mtm<D, T>(bRR, 1.0, SS, bP);
      add_mmt<D, T>(bRR, 1.0, bQ, SS);
      add_mtm<D, T>(bSS, 1.0, RR, bQ);
    }
    if (HASV) {
      adiag<D, T>(bSS, vb[0]);      // V0 = tr SS
      adiag<D, T>(bRR, vb[1]);      // V1 = tr RR
      axpyT<D, T>(bSS, vb[2], S);   // V2 = tr(SS·S)
      axpyT<D, T>(bS, vb[2], SS);
      axpyT<D, T>(bS, vb[3], RR);   // V3 = tr(S·RR)
      axpyT<D, T>(bRR, vb[3], S);
    }
    add_mmt<D, T>(bS, 1.0, bSS, S);  // SS = S·S
    add_mtm<D, T>(bS, 1.0, S, bSS);
    add_mmt<D, T>(bR, 1.0, bRR, R);  // RR = R·R
    add_mtm<D, T>(bR, 1.0, R, bRR);
  }
  add_mmt<D, T>(bS, 1.0, bSR, R);  // SR = S·R
  add_mtm<D, T>(bR, 1.0, S, bSR);
  add_mmt<D, T>(bR, 1.0, bRS, S);  // RS = R·S
  add_mtm<D, T>(bS, 1.0, R, bRS);
}

// ∇ubar = sym(Sbar) + skew(Rbar) into the scratch: entry (a, b) at field a·D + b
template <int D, typename T>
__device__ __forceinline__ void put_gradbar(const GridDev& g, T* __restrict__ gb, long long c, const Mat<D, T>& bS, const Mat<D, T>& bR) {
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) gb[(long long)(a * D + b) * g.sc + c] = (bS.m[a][b] + bS.m[b][a]) / 2 + (bR.m[a][b] - bR.m[b][a]) / 2;
}

// The symmetric D×D matrix M with <M, B> = Σ_{a<=b} t_ab B_ab for symmetric B: the cotangent of the D(D+1)/2 stored entries of τ
template <int D, typename T>
__device__ __forceinline__ Mat<D, T> full_cotangent(const GridDev& g, const T* __restrict__ t, long long c) {
  Mat<D, T> M;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) M.m[a][b] = T(a == b ? 1.0 : 0.5) * t[(long long)sym_index<D>(a, b) * g.sc + c];
  return M;
}

// --------------------------------------------------------------------------------------------
// forward: invariants and fused stress (write Ip)
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_tc_invariants(GridDev g, const T* __restrict__ u, T* __restrict__ V) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  T v[5];
  invariants<D, T>(S, R, v);
  constexpr int nv = D == 2 ? 2 : 5;
#pragma unroll
  for (int q = 0; q < nv; ++q) V[q * g.sc + c] = v[q];
}

template <int D, typename T>
__global__ __launch_bounds__(256) void k_tc_stress(GridDev g, const T* __restrict__ u, const T* __restrict__ a, T* __restrict__ tau) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  Mat<D, T> M = mzero<D, T>();
  for_each_basis<D, T>(S, R, [&](int ib, const Mat<D, T>& B) { axpy<D, T>(M, a[ib * g.sc + c], B); });
#pragma unroll
  for (int p = 0; p < D; ++p)
#pragma unroll
    for (int q = p; q < D; ++q) tau[(long long)sym_index<D>(p, q) * g.sc + c] = M.m[p][q];
}

// smagtensor! (operators.jl:1135-1150) on the pointwise gradient above: σ = 2 νt S with νt = θ² Δ² sqrt(2 S:S), Δ² = Σ Δα² (gridsize), written on Ip
// as D(D+1)/2 fields.  The expressions of gradient_result<D, 2> in ins_fields.hip, whose register-row and LDS-ring kernels serve fp64 only.
// WARNING: a copy, not an instantiation, of that fp64 code: a fix to one goes into the other as well (ins_fields.hip says why).
template <int D, typename T>
__global__ __launch_bounds__(256) void k_smagtensor(GridDev g, T theta, const T* __restrict__ u, T* __restrict__ sig) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  T d2 = T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) d2 += (T)g.dx[a][I[a]] * (T)g.dx[a][I[a]];
  const T eddy = theta * theta * d2 * sqrt(2 * mdot<D, T>(S, S));
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = a; b < D; ++b) sig[(long long)sym_index<D>(a, b) * g.sc + c] = 2 * eddy * S.m[a][b];
}

// --------------------------------------------------------------------------------------------
// pass 1 of the pullbacks: ∇ubar at every pressure point
// --------------------------------------------------------------------------------------------
// abar_i = <τbar, B_i> over the whole padded array (0 outside Ip, where the forward reads no a)
template <int D, typename T>
__global__ __launch_bounds__(256) void k_tc_abar(GridDev g, const T* __restrict__ u, const T* __restrict__ taubar, T* __restrict__ abar) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
  constexpr int nb = D == 2 ? 3 : 11;
  if (!in_ip<D>(g, i, j, k)) {
#pragma unroll
    for (int ib = 0; ib < nb; ++ib) abar[ib * g.sc + c] = T(0);
    return;
  }
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  const Mat<D, T> M = full_cotangent<D, T>(g, taubar, c);
  for_each_basis<D, T>(S, R, [&](int ib, const Mat<D, T>& B) { abar[ib * g.sc + c] = mdot<D, T>(M, B); });
}

// closure route: Bbar_i = a_i τbar, plus the invariants' cotangent
template <int D, typename T, bool HASA, bool HASV>
__global__ __launch_bounds__(256) void k_tc_gradbar(GridDev g, const T* __restrict__ u, const T* __restrict__ a, const T* __restrict__ taubar,
                                                    const T* __restrict__ Vbar, T* __restrict__ gb) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  T vb[5] = {0, 0, 0, 0, 0};
  constexpr int nv = D == 2 ? 2 : 5;
  if (HASV) {
#pragma unroll
    for (int q = 0; q < nv; ++q) vb[q] = Vbar[q * g.sc + c];
  }
  Mat<D, T> tb = mzero<D, T>();
  if (HASA) tb = full_cotangent<D, T>(g, taubar, c);
  Mat<D, T> bS, bR;
  basis_reverse<D, T, HASA, HASV>(S, R, [&](int ib) {
    Mat<D, T> M = tb;
    const T s = a[ib * g.sc + c];
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int q = 0; q < D; ++q) M.m[p][q] *= s;
    return M; }, vb, bS, bR);
  put_gradbar<D, T>(g, gb, c, bS, bR);
}

// operator route: Bbar in the layout of ins_tensorbasis_f64 (element (p, q) of tensor ib at field ib·D·D + p + D·q)
template <int D, typename T, bool HASB, bool HASV>
__global__ __launch_bounds__(256) void k_tb_gradbar(GridDev g, const T* __restrict__ u, const T* __restrict__ Bbar, const T* __restrict__ Vbar,
                                                    T* __restrict__ gb) {
  INS_VOL_INDEX(g.sx, g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], !in_ip<D>(g, i, j, k));
  Mat<D, T> S, R;
  strain_rotation<D, T>(g, u, c, I, S, R);
  T vb[5] = {0, 0, 0, 0, 0};
  constexpr int nv = D == 2 ? 2 : 5;
  if (HASV) {
#pragma unroll
    for (int q = 0; q < nv; ++q) vb[q] = Vbar[q * g.sc + c];
  }
  Mat<D, T> bS, bR;
  basis_reverse<D, T, HASB, HASV>(S, R, [&](int ib) {
    Mat<D, T> M;
#pragma unroll
    for (int p = 0; p < D; ++p)
#pragma unroll
      for (int q = 0; q < D; ++q) M.m[p][q] = Bbar[(long long)(ib * D * D + p + D * q) * g.sc + c];
    return M; }, vb, bS, bR);
  put_gradbar<D, T>(g, gb, c, bS, bR);
}

}  // namespace
