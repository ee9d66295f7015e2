// DNS-to-LES filters of lib/NeuralClosure (filter.jl): face average, volume average, reconstruction, and the exact
// transposes of the two filters, once for both precisions: templates over the scalar type T of the fields, instantiated with
// double by ins_filter.hip and with float by ins_filter32.hip (two translation units, as ins_fields_kernels.h).  2-D and 3-D.
//
// A coarse ("LES") and a fine ("DNS") grid are two handles with n_dns = comp·n_les interior volumes per direction and
// nested faces.  All indices below are 0-based positions in the padded arrays (N = n + ghosts, x fastest).
//
//   face    v[I, α] = mean of u[f, α],  f_α = lo_α + comp·(I_α − lo_α) + comp − 1,  f_β = lo_β + comp·(I_β − lo_β) + 0..comp−1   (β ≠ α)
//           for I ∈ Iu[α] of the coarse grid, lo = first index of Iu[α]                                            filter.jl:26-46
//   volume  v[I, α] = mean of u[f, α],  f_α = comp·I_α − h .. comp·I_α + h  (h = comp/2: comp + 1 planes for even comp, comp for odd),
//           f_β = comp·(I_β − 1) + 1..comp, f wrapped into the fine interior 1..n_dns; all-periodic grids           filter.jl:82-116
//   reconstruct  u[f, α] = ((comp − i_α)·v[c, α] + i_α·v[c − e_α, α]) / comp,  c = ceil(f / comp),  i = comp·c − f,
//           c − e_α wrapped into the coarse interior; all-periodic grids                                            filter.jl:48-80
//
// The filters write Iu[α] of the coarse field only; reconstruct writes the fine interior only.  The pullbacks overwrite the whole padded
// fine cotangent (zeros where the forward reads nothing), gather form, no atomics, as ins_adjoint.hip.
//
// Precision.  Loads and stores are T.  Every window sum, the reconstruct interpolation and the pullback gather are formed in double and
// rounded once at the store (the LDS row of the tiled kernel is double too): with T = double this is the arithmetic the kernels had when they
// were written in double inside ins_filter.hip, same order of summation, same sum / cnt; with T = float every output is the rounded value of a
// double result whose own error is n·eps64, far below half a float ulp.  The kernels are bound by their loads, so the wider
// accumulator costs nothing.
//
// Two kernels serve the filters: a generic one (one coarse face per work-item, every case) and a tiled one for the case that matters, a 3-D
// all-periodic box with comp ∈ {2, 4, 8} (the fp64 face average from comp = 4): a wavefront reads whole contiguous fine x-rows (W volumes per lane),
// sums the y and z window in registers, and reduces the x window over an LDS row.  INS_DISABLE_FILTER_TILED forces the generic kernel for both
// precisions.
#pragma once

#include <cmath>

#include "ins_stencil.h"

namespace {

struct FilterArgs {
  int comp;
  int Nc[3], Nf[3];  // padded sizes
  int nf[3], nc[3];  // interior volumes (periodic wrap length)
  long long sxc[3], scc, sxf[3], scf;
  int lo[3][3], hi[3][3];  // coarse Iu[α] in direction β
};

// --------------------------------------------------------------------------------------------
// generic filters: one work-item per coarse volume, all components
// --------------------------------------------------------------------------------------------
// The window sums of coarse volume I (linear index c) for every component: the one text of the generic filters.  mu / mv: element offsets of the member of
// an ensemble this work-item works on (k_filter_members); the single-field kernel passes the constant 0, which folds away.
template <int D, bool VOL, typename T>
__device__ __forceinline__ void filter_faces(const FilterArgs& a, const int (&I)[3], const long long c, const T* __restrict__ ufield, T* __restrict__ vfield,
                                             const long long mu, const long long mv) {
  const int C = a.comp;
  const int h = C / 2;
#pragma unroll
  for (int al = 0; al < D; ++al) {
    bool in = true;
    int s[3] = {0, 0, 0}, n[3] = {1, 1, 1};
#pragma unroll
    for (int b = 0; b < D; ++b) {
      in = in && I[b] >= a.lo[al][b] && I[b] < a.hi[al][b];
      if (VOL) {
        s[b] = b == al ? C * I[b] - h : C * (I[b] - 1) + 1;
        n[b] = b == al ? (C % 2 == 0 ? C + 1 : C) : C;
      } else {
        s[b] = a.lo[al][b] + C * (I[b] - a.lo[al][b]) + (b == al ? C - 1 : 0);
        n[b] = b == al ? 1 : C;
      }
    }
    if (!in) continue;
    const double cnt = (double)(n[0] * n[1] * n[2]);
    const T* __restrict__ u = ufield + mu + al * a.scf;
    double sum = 0.0;
    for (int q2 = 0; q2 < n[2]; ++q2) {
      int f2 = s[2] + q2;
      if (VOL && D == 3 && f2 > a.nf[2]) f2 -= a.nf[2];
      for (int q1 = 0; q1 < n[1]; ++q1) {
        int f1 = s[1] + q1;
        if (VOL && f1 > a.nf[1]) f1 -= a.nf[1];
        const long long row = f1 * a.sxf[1] + f2 * a.sxf[2];
        for (int q0 = 0; q0 < n[0]; ++q0) {
          int f0 = s[0] + q0;
          if (VOL && f0 > a.nf[0]) f0 -= a.nf[0];
          sum += (double)u[row + f0];
        }
      }
    }
    vfield[mv + al * a.scc + c] = (T)(sum / cnt);
  }
}

template <int D, bool VOL, typename T>
__global__ __launch_bounds__(256) void k_filter(FilterArgs a, const T* __restrict__ ufield, T* __restrict__ vfield) {
  INS_VOL_INDEX(a.sxc, 0, 0, 0, i >= a.Nc[0] || j >= a.Nc[1]);
  filter_faces<D, VOL, T>(a, I, c, ufield, vfield, 0LL, 0LL);
}

// The same sums for member blockIdx.z of an ensemble of 2-D fields (in 2-D INS_VOL_INDEX leaves blockIdx.z unused): member b of the fine fields lies
// b·ustride elements behind ufield, of the coarse fields b·vstride behind vfield.  One launch for all members; the tiles are the single field's.
template <bool VOL, typename T>
__global__ __launch_bounds__(256) void k_filter_members(FilterArgs a, const T* __restrict__ ufield, long long ustride, T* __restrict__ vfield,
                                                        long long vstride) {
  constexpr int D = 2;
  INS_VOL_INDEX(a.sxc, 0, 0, 0, i >= a.Nc[0] || j >= a.Nc[1]);
  const long long b = blockIdx.z;
  filter_faces<2, VOL, T>(a, I, c, ufield, vfield, b * ustride, b * vstride);
}

// --------------------------------------------------------------------------------------------
// tiled filters: 3-D, all-periodic, comp = C ∈ {2, 4, 8}.  Block = 4 wavefronts = 4 coarse y-rows of one coarse z-plane; a wavefront owns
// 64·W contiguous fine x-volumes (fine index 64·W·bx + 1 + W·lane + 0..W−1) = 64·W/C coarse outputs.  Every load is one whole row segment of
// 64·W·sizeof(T) bytes; the α = x component of the face average needs one volume in C of them and loads the whole row all the same (every cache
// line of the row is touched either way).  W = 2 is the float form: the lane's pair starts at padded index 1 + 2·lane, so it is
// 4-byte aligned, not 8 — FilterPair below says so, and the load is one 8-byte instruction that the hardware takes at dword alignment.
// --------------------------------------------------------------------------------------------
template <typename T, int W>
struct __attribute__((packed, aligned(sizeof(T)))) FilterPair {
  T x[W];
};

template <int C, bool VOL, int AL, typename T, int W>
__device__ __forceinline__ void tiled_component(const FilterArgs& a, const T* __restrict__ ufield, T* __restrict__ vfield, double* t, int bx, int Jc,
                                                int Kc, bool rowok) {
  constexpr int TILE = 64 * W;
  constexpr int H = C / 2;
  constexpr int NY = VOL ? (AL == 1 ? C + 1 : C) : (AL == 1 ? 1 : C);
  constexpr int NZ = VOL ? (AL == 2 ? C + 1 : C) : (AL == 2 ? 1 : C);
  const int lane = threadIdx.x;
  const int n0 = a.nf[0];
  const int valid = min(TILE, n0 - TILE * bx);  // fine volumes of this tile (a multiple of C, so of W: C is even)
  const int sy = VOL ? (AL == 1 ? C * Jc - H : C * (Jc - 1) + 1) : (AL == 1 ? C * Jc : C * (Jc - 1) + 1);
  const int sz = VOL ? (AL == 2 ? C * Kc - H : C * (Kc - 1) + 1) : (AL == 2 ? C * Kc : C * (Kc - 1) + 1);
  const T* __restrict__ u = ufield + AL * a.scf;
  const bool main_ok = rowok && W * lane < valid;
  const bool halo_ok = VOL && AL == 0 && rowok && lane < H;  // the x window of the last output reaches H volumes into the next tile
  int ih = TILE * bx + 1 + valid + lane;
  if (ih > n0) ih -= n0;
  const int i = TILE * bx + 1 + W * lane;
  double acc[W], acch = 0.0;
#pragma unroll
  for (int q = 0; q < W; ++q) acc[q] = 0.0;
#pragma unroll
  for (int qz = 0; qz < NZ; ++qz) {
    int fz = sz + qz;
    if (VOL && fz > a.nf[2]) fz -= a.nf[2];
#pragma unroll
    for (int qy = 0; qy < NY; ++qy) {
      int fy = sy + qy;
      if (VOL && fy > a.nf[1]) fy -= a.nf[1];
      const long long row = fy * a.sxf[1] + fz * a.sxf[2];
      if (main_ok) {
        const FilterPair<T, W> p = *reinterpret_cast<const FilterPair<T, W>*>(u + row + i);
#pragma unroll
        for (int q = 0; q < W; ++q) acc[q] += (double)p.x[q];
      }
      if (halo_ok) acch += (double)u[row + ih];
    }
  }
  if (main_ok) {
#pragma unroll
    for (int q = 0; q < W; ++q) t[W * lane + q] = acc[q];
  }
  if (halo_ok) t[valid + lane] = acch;
  __syncthreads();
  if (rowok && lane < valid / C) {
    double s = 0.0;
    if (VOL && AL == 0) {
#pragma unroll
      for (int q = -H; q <= H; ++q) s += t[C * (lane + 1) - 1 + q];
    } else if (AL == 0) {
      s = t[C * (lane + 1) - 1];
    } else {
#pragma unroll
      for (int q = 0; q < C; ++q) s += t[C * lane + q];
    }
    constexpr double cnt = VOL ? (double)((C + 1) * C * C) : (double)(C * C);
    vfield[AL * a.scc + (TILE * bx / C + 1 + lane) + Jc * a.sxc[1] + Kc * a.sxc[2]] = (T)(s / cnt);
  }
}

template <int C, bool VOL, typename T, int W>
__global__ __launch_bounds__(256) void k_filter_tiled(FilterArgs a, const T* __restrict__ u, T* __restrict__ v) {
  __shared__ double lds[3][4][64 * W + 4];  // one row per component and wavefront: no row is reused, so one barrier per component
  const int bx = blockIdx.x;
  const int Jc = blockIdx.y * 4 + threadIdx.y + 1;
  const int Kc = blockIdx.z + 1;
  const bool rowok = Jc <= a.nc[1];
  tiled_component<C, VOL, 0, T, W>(a, u, v, lds[0][threadIdx.y], bx, Jc, Kc, rowok);
  tiled_component<C, VOL, 1, T, W>(a, u, v, lds[1][threadIdx.y], bx, Jc, Kc, rowok);
  tiled_component<C, VOL, 2, T, W>(a, u, v, lds[2][threadIdx.y], bx, Jc, Kc, rowok);
}

// --------------------------------------------------------------------------------------------
// reconstruct: one work-item per fine volume (interior only)
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_reconstruct(FilterArgs a, const T* __restrict__ v, T* __restrict__ u) {
  INS_VOL_INDEX(a.sxf, 0, 0, 0, false);
  bool in = true;
#pragma unroll
  for (int b = 0; b < D; ++b) in = in && I[b] >= 1 && I[b] <= a.nf[b];
  if (!in) return;
  const int C = a.comp;
  int ci[3] = {0, 0, 0}, off[3] = {0, 0, 0};
  long long cc = 0;
#pragma unroll
  for (int b = 0; b < D; ++b) {
    ci[b] = (I[b] + C - 1) / C;
    off[b] = C * ci[b] - I[b];
    cc += ci[b] * a.sxc[b];
  }
#pragma unroll
  for (int al = 0; al < D; ++al) {
    const int cl = ci[al] == 1 ? a.nc[al] : ci[al] - 1;
    const long long cleft = cc + (long long)(cl - ci[al]) * a.sxc[al];
    double s = 0.0;
    s += (double)(C - off[al]) * (double)v[al * a.scc + cc];
    s += (double)off[al] * (double)v[al * a.scc + cleft];
    u[al * a.scf + c] = (T)(s / (double)C);
  }
}

// --------------------------------------------------------------------------------------------
// pullbacks: one work-item per fine volume of the whole padded array; ubar = Φᵀ w
// --------------------------------------------------------------------------------------------
template <int D, typename T>
__global__ __launch_bounds__(256) void k_filter_face_pullback(FilterArgs a, const T* __restrict__ w, T* __restrict__ ubar) {
  INS_VOL_INDEX(a.sxf, 0, 0, 0, i >= a.Nf[0] || j >= a.Nf[1]);
  const int C = a.comp;
  double cnt = 1.0;
  for (int b = 1; b < D; ++b) cnt *= (double)C;
#pragma unroll
  for (int al = 0; al < D; ++al) {
    bool hit = true;
    long long cc = 0;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const int q = I[b] - a.lo[al][b] - (b == al ? C - 1 : 0);
      hit = hit && q >= 0 && (b != al || q % C == 0);
      const int Ic = a.lo[al][b] + (q >= 0 ? q / C : 0);
      hit = hit && Ic < a.hi[al][b];
      cc += Ic * a.sxc[b];
    }
    ubar[al * a.scf + c] = hit ? (T)((double)w[al * a.scc + cc] / cnt) : T(0);
  }
}

template <int D, typename T>
__global__ __launch_bounds__(256) void k_filter_volume_pullback(FilterArgs a, const T* __restrict__ w, T* __restrict__ ubar) {
  INS_VOL_INDEX(a.sxf, 0, 0, 0, i >= a.Nf[0] || j >= a.Nf[1]);
  const int C = a.comp;
  const int h = C / 2;
  bool in = true;
  int ct[3] = {0, 0, 0};  // coarse volume whose tangential window holds F
#pragma unroll
  for (int b = 0; b < D; ++b) {
    in = in && I[b] >= 1 && I[b] <= a.nf[b];
    ct[b] = (I[b] + C - 1) / C;
  }
  double cnt = (double)(C % 2 == 0 ? C + 1 : C);
  for (int b = 1; b < D; ++b) cnt *= (double)C;
#pragma unroll
  for (int al = 0; al < D; ++al) {
    double s = 0.0;
    if (in) {
      long long base = 0;
#pragma unroll
      for (int b = 0; b < D; ++b)
        if (b != al) base += ct[b] * a.sxc[b];
      // coarse faces comp·Ic within h of I[al] (periodic): at most two, and two only for even comp at the shared plane
      const int q = I[al] / C, r = I[al] % C;
      if (r <= h) {
        const int Ic = q == 0 ? a.nc[al] : q;
        s += (double)w[al * a.scc + base + Ic * a.sxc[al]];
      }
      if (C - r <= h) {
        const int Ic = q + 1 > a.nc[al] ? 1 : q + 1;
        s += (double)w[al * a.scc + base + Ic * a.sxc[al]];
      }
    }
    ubar[al * a.scf + c] = (T)(s / cnt);
  }
}

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
inline int ghosts_left(const ins_grid* G, int b) { return G->desc.bc[b][0] == INS_BC_PRESSURE ? 2 : 1; }

// Checks the pair of grids and fills the arguments.  `need_periodic`: volume average / reconstruct.
inline int prepare(const ins_grid* les, const ins_grid* dns, int comp, bool need_periodic, const char* what, FilterArgs& a) {
  INS_REQUIRE(les && dns, "null grid handle");
  INS_REQUIRE(comp >= 1, "compression must be >= 1");
  const int D = les->g.D;
  INS_REQUIRE(dns->g.D == D, "the two grids differ in dimension");
  memset(&a, 0, sizeof(a));
  a.comp = comp;
  for (int b = 0; b < 3; ++b) {
    a.Nc[b] = les->g.N[b];
    a.Nf[b] = dns->g.N[b];
    a.sxc[b] = les->g.sx[b];
    a.sxf[b] = dns->g.sx[b];
    a.nc[b] = a.nf[b] = 1;
  }
  a.scc = les->g.sc;
  a.scf = dns->g.sc;
  for (int b = 0; b < D; ++b) {
    for (int s = 0; s < 2; ++s) INS_REQUIRE(les->desc.bc[b][s] == dns->desc.bc[b][s], "the two grids differ in boundary conditions");
    const int gl = ghosts_left(les, b);
    a.nc[b] = les->g.N[b] - gl - 1;
    a.nf[b] = dns->g.N[b] - gl - 1;
    INS_REQUIRE((long long)comp * a.nc[b] == a.nf[b], "n_dns must be comp * n_les in every direction");
    // nested faces: every coarse volume is the union of its comp fine volumes
    for (int I = 0; I < a.nc[b]; ++I) {
      double sum = 0.0;
      for (int q = 0; q < comp; ++q) sum += dns->desc.dx[b][gl + comp * I + q];
      const double w = les->desc.dx[b][gl + I];
      INS_REQUIRE(std::fabs(sum - w) <= 1e-8 * std::fabs(w), "the grids are not nested (x_les[i] != x_dns[comp*i])");
    }
  }
  for (int al = 0; al < D; ++al)
    for (int b = 0; b < D; ++b) {
      a.lo[al][b] = les->g.iu_lo[al][b];
      a.hi[al][b] = les->g.iu_hi[al][b];
      // last fine index the face average reads
      const long long last = a.lo[al][b] + (long long)comp * (a.hi[al][b] - 1 - a.lo[al][b]) + comp - 1;
      INS_REQUIRE(last <= dns->g.N[b] - 1, "the face window leaves the fine array");
    }
  if (need_periodic && !(les->all_periodic && dns->all_periodic)) {
    ins_set_error("%s needs an all-periodic grid", what);
    return INS_ERR_UNSUPPORTED;
  }
  return INS_OK;
}

// The face average at comp = 2 is routed by measurement: in fp64 it stays on the generic kernel (equal at 256³, tiled 10 % slower at
// 512³); in float, with two volumes per lane, the tiled kernel is 21 % (256³) and 16 % (512³) faster, so `face2` (the float entries) takes it.
inline bool tiled_supported(const ins_grid* les, const ins_grid* dns, int comp, bool vol, bool face2) {
  return les->g.D == 3 && les->all_periodic && dns->all_periodic && (comp == 4 || comp == 8 || (comp == 2 && (vol || face2))) &&
         !ins_opt(OPT_INS_DISABLE_FILTER_TILED);
}

// W: fine x-volumes per lane of the tiled kernel
template <bool VOL, typename T, int W>
int launch_filter(const ins_grid* les, const ins_grid* dns, int comp, const T* u, T* v, hipStream_t s) {
  FilterArgs a;
  int rc = prepare(les, dns, comp, VOL, VOL ? "the volume average" : "the face average", a);
  if (rc) return rc;
  INS_REQUIRE(u && v, "null field");
  INS_REQUIRE(u != v, "the filter cannot run in place");
  const GridDev& g = les->g;
  if (tiled_supported(les, dns, comp, VOL, sizeof(T) == sizeof(float))) {
    dim3 block(64, 4, 1), grid(cdiv(a.nf[0], 64 * W), cdiv(a.nc[1], 4), (unsigned)a.nc[2]);
    if (comp == 2)
      hipLaunchKernelGGL((k_filter_tiled<2, VOL, T, W>), grid, block, 0, s, a, u, v);
    else if (comp == 4)
      hipLaunchKernelGGL((k_filter_tiled<4, VOL, T, W>), grid, block, 0, s, a, u, v);
    else
      hipLaunchKernelGGL((k_filter_tiled<8, VOL, T, W>), grid, block, 0, s, a, u, v);
    INS_LAUNCH_CHECK();
  } else {
    INS_LAUNCH_D((k_filter<D, VOL, T>), box_launch(g.D, a.Nc), s, a, u, v);
  }
  return INS_OK;
}

// nbatch 2-D fields in one launch of the generic kernel's text (k_filter_members).  Member b of the fine fields lies at u + b·ustride (ustride >= 2·ncell of the
// fine grid), of the coarse fields at v + b·vstride; what lies between members is neither read nor written.
template <bool VOL, typename T>
int launch_filter_members(const ins_grid* les, const ins_grid* dns, int comp, int nbatch, const T* u, long long ustride, T* v, long long vstride,
                          hipStream_t s) {
  INS_REQUIRE(les && dns, "null grid handle");
  if (les->g.D != 2 || dns->g.D != 2) {
    ins_set_error("ins_filter_%s_members_f64: a 3-D grid; the member form of the filters runs 2-D grids only: filter each member with ins_filter_%s_f64",
                  VOL ? "volume" : "face", VOL ? "volume" : "face");
    return INS_ERR_UNSUPPORTED;
  }
  FilterArgs a;
  int rc = prepare(les, dns, comp, VOL, VOL ? "the volume average" : "the face average", a);
  if (rc) return rc;
  INS_REQUIRE(u && v, "null field");
  INS_REQUIRE((const void*)u != (const void*)v, "the filter cannot run in place");
  INS_REQUIRE(nbatch >= 1 && nbatch <= 65535, "an ensemble has 1 .. 65535 members");
  INS_REQUIRE(ustride >= 2 * dns->ncell, "member stride of the fine fields shorter than a vector field (2 ncell)");
  INS_REQUIRE(vstride >= 2 * les->ncell, "member stride of the coarse fields shorter than a vector field (2 ncell)");
  Launch3 l = box_launch(2, a.Nc);
  l.grid.z = (unsigned)nbatch;
  hipLaunchKernelGGL((k_filter_members<VOL, T>), l.grid, l.block, 0, s, a, u, ustride, v, vstride);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

template <typename T>
int launch_reconstruct(const ins_grid* dns, const ins_grid* les, int comp, const T* v, T* u, hipStream_t s) {
  FilterArgs a;
  int rc = prepare(les, dns, comp, true, "reconstruct", a);
  if (rc) return rc;
  INS_REQUIRE(u && v && u != v, "null or aliased field");
  const GridDev& g = les->g;
  INS_LAUNCH_D((k_reconstruct<D, T>), box_launch(g.D, a.Nf), s, a, v, u);
  return INS_OK;
}

template <bool VOL, typename T>
int launch_filter_pullback(const ins_grid* les, const ins_grid* dns, int comp, const T* w, T* ubar, hipStream_t s) {
  FilterArgs a;
  int rc = prepare(les, dns, comp, VOL, VOL ? "the volume average" : "the face average", a);
  if (rc) return rc;
  INS_REQUIRE(w && ubar && w != ubar, "null or aliased field");
  const GridDev& g = les->g;
  if (VOL) {
    INS_LAUNCH_D((k_filter_volume_pullback<D, T>), box_launch(g.D, a.Nf), s, a, w, ubar);
  } else {
    INS_LAUNCH_D((k_filter_face_pullback<D, T>), box_launch(g.D, a.Nf), s, a, w, ubar);
  }
  return INS_OK;
}

}  // namespace
