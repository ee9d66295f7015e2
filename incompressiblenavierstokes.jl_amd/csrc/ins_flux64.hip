// K1 (flux form, 64 outputs per wavefront) — the periodic / exactly-uniform specialisation of ins_fast3d_flux.hip
// (convection_diffusion_kernel! + fill!(F, 0), operators.jl:647-690, 971; optional RK epilogue and in-register
// pressure correction exactly as documented there).
//
// ins_fast3d_flux.hip spends lanes 0 and 63 of every wavefront on halo columns, so a 256-wide row needs 5 wavefronts
// (62+62+62+62+8) and a 512-wide row 9.  Here all 64 lanes produce output:
//   * the two halo columns (x0-1 and x0+64) of ALL R+2 rows arrive in ONE extra load per component and plane, rows
//     packed across lanes (lanes 0..7: left column, lanes 16..23: right column);
//   * `v_readlane` moves a packed halo value to an SGPR; it enters the wave shift as the DPP `old` operand, i.e. the value
//     lane 63 (wave_shl) or lane 0 (wave_shr) keeps when it has no source lane;
//   * lane 0 has no left neighbour to take the left-face x-fluxes from: they are evaluated from the halo scalars (three
//     more flux evaluations per row, wave-wide; the kernel is memory-bound);
//   * with the pressure correction (CORR) the packed halo columns are corrected in packed form from a packed load of the
//     four pressure columns x0-1, x0, x0+64, x0+65 (DPP row shifts inside the 16-lane rows).
// So every column of u is loaded once per (R+2)-row window and a 256 (512) wide row takes exactly 4 (8) wavefronts.
// Everything else (R+2 register rows, z-march with carried z-flux, 3-buffer plane prefetch, k-major XCD-partitioned tile
// order) is the scheme of ins_fast3d_flux.hip.  Addressing: wave-uniform row bases (SGPR) + one 32-bit lane offset, so the
// loads use the saddr form and no 64-bit address registers; the grid enters as 12 scalars instead of the GridDev tables.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ins_debug.h"
#include "ins_f32_internal.h"
#include "ins_wave64.h"
#include "ins_flux_common.h"

namespace {

template <typename T, int R>
struct Plane {
  T v[3][R + 2];
  T h[3];  // packed halo columns: lane r = row r of column x0-1, lane 16+r = row r of column x0+64
  T raw[3][R];  // CORR: the output rows before the pressure correction (a term of the stage-velocity basis, ins_rk.hip)
  T vm2;        // RHS: the y-component at row jb0-2 (the y-flux below the row whose v* the first output row's divergence needs)
  T rawv0;      // RHS, CORR: the y-component at row jb0-1 before the pressure correction
};

// temperature rows of a register plane (EXTRA, a.tm): T rides along as a fourth component; vm1 = the y-component at the row BELOW the halo
// row (the Laplacian of v at the halo row needs it: dissipation! reads u·diffusion(u) of the volume below)
template <typename T, int R>
struct TExt {
  T t[R + 2];
  T th;  // packed halo columns of T
  T vm1;
};

// NW wavefronts per workgroup: XW side by side in x, NW/XW stacked in y.  CORR as in ins_fast3d_flux.hip: 0 = `u` has valid ghost volumes;
// 1 = `u` is the previous stage's uncorrected u* (interior only), pI its unpadded pressure, every neighbour through the
// periodic image; 2 = z-slab: x, y periodic images, z through exchanged ghost planes, pI = [1 | nzl | 2] extended buffer.
// EXTRA (extended stage loop, ins_rk_ext.hip): epi.extra is a vector field added to the stage force before it is used and stored
// (k_i = F_i + closure(u_i) + gravity(temp_i), step_explicit_runge_kutta.jl:21-34).
// RHS (workgroups that span whole rows, 64 XW == n0; CORR 0 / 1): the kernel also stores the Poisson right-hand side Ω·div(u*) of the stage velocity
// it writes, into a.epi.rhs_out (unpadded, the layout k_xfwd<XSRC_PI> reads), so the x-forward pass reads one scalar array instead of three components.
// The three lower neighbours of a cell's divergence:
//   x  u*(i-1): the wave shift; lane 0 takes lane 63 of the wavefront to the left (periodic inside the workgroup) through LDS.  The workgroup's one
//      barrier per plane moves from the top of the plane to between the LDS write and the LDS read (two LDS slots, alternating by plane);
//   y  v*(jb0-1), the row below the wavefront's first output row, belongs to another wavefront: it is computed here again, from the same expressions
//      in the same order (so it is the value that wavefront stores): one more y-flux (row jb0-2 of v, of p), the v terms of the epilogue at row jb0-1;
//   z  w*(k-1) is carried along the march; the march starts one plane early (k0-1, nothing stored) so the first plane of a chunk has it.
// CARRY (CORR 1, a.epi.carry_out; ins_rk_terms.h, RkCarryPlan): the kernel also stores S = ca0·s + ca1·raw + ca2·u* at the cells it stores u* at, s = the
// combination before coef_self·f is added, raw = the uncorrected stencil input (kept alive to the stores: 12 more registers, hence a flag of its own).
// XF (RHS, CORR 1, fp64, 2 rows, 4 wavefronts per 256-wide row; a.epi.spec_out instead of rhs_out): the kernel stores the half-complex x-spectrum of that right-hand
// side, the array k_xfwd<8, 4, XSRC_PI> would make of it, and the solve starts at its y pass.  After the plane's barrier a lane holds one point of k_xfwd's packing,
// z[i] = (rhs(i, jb0), rhs(i, jb0+1)), i = 64 wx + lane.  The first radix-4 stage of the 256-point decimation-in-frequency transform joins the same lane of the four
// wavefronts of a row and leaves branch wx in wavefront wx; the other three stages are a 64-point transform inside one wavefront (no workgroup barrier); frequency s
// ends at position digit-reverse(s) (pos_of_freq<8>, ins_fft.hip).  To keep the one barrier per plane the transform lags: iteration k, behind its barrier,
//   A  writes z of plane k to X1[k & 1];
//   B  reads the four first-stage inputs of plane k-1 from X1[(k-1) & 1] (written before this barrier), does output wx of the butterfly, runs the three wave-local stages
//      in place in the wavefront's own quarter of X2[(k-1) & 1] (one point per lane: four reads and one write per stage, ordered by the LDS queue of the wavefront);
//   C  reads Z[pos(s)], Z[pos(N-s)] of plane k-2 from X2[k & 1] (finished before this barrier), separates the two real rows and stores them.
// Every slot is written again two iterations later, behind the next barrier.  Two drain iterations end a chunk; the plane below the chunk enters nothing.
// The finished transform is stored rotated inside groups of 16 (fft_swz, ins_fft.hip: the reads of step C are 1 KB apart otherwise).  The per-lane twiddles (w^m of each stage, the products
// k_xfwd forms) are computed once and read back per plane from LDS, each lane its own entry: 12 registers less across the march.
struct Xc {
  double x, y;
};
__device__ __forceinline__ Xc xc_mul(Xc a, Xc b) { return Xc{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
// output m of the radix-4 decimation-in-frequency butterfly (fft_dif, ins_fft.hip): 0: (a0+a2)+(a1+a3), 1: (a0-a2)-i(a1-a3), 2: (a0+a2)-(a1+a3), 3: (a0-a2)+i(a1-a3)
__device__ __forceinline__ Xc xc_bfly(Xc a0, Xc a1, Xc a2, Xc a3, int m) {
  const bool odd = m & 1, neg = m & 2;
  const double s2 = odd ? -1.0 : 1.0;  // (a sign flip is exact: the sums round as the differences do)
  const Xc p{a0.x + s2 * a2.x, a0.y + s2 * a2.y}, q0{a1.x + s2 * a3.x, a1.y + s2 * a3.y};
  Xc q = odd ? Xc{q0.y, -q0.x} : q0;
  const double s1 = neg ? -1.0 : 1.0;
  return Xc{p.x + s1 * q.x, p.y + s1 * q.y};
}
__device__ __forceinline__ int xf_swz(int i) { return (i & ~15) | ((i + ((i >> 4) & 3) + 4 * ((i >> 6) & 3)) & 15); }
__device__ __forceinline__ int xf_pos(int s) { return ((s & 3) << 6) | (((s >> 2) & 3) << 4) | (((s >> 4) & 3) << 2) | ((s >> 6) & 3); }  // pos_of_freq<8>
__device__ __forceinline__ void xf_wave_sync() {  // LDS writes of this wavefront before its later LDS reads (program order in the LDS queue; this pins the compiler)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

template <typename T, int R, int XW, bool FUSE, int CORR, bool SKEL = false, int NW = 4, bool EXTRA = false, bool RHS = false, bool CARRY = false, bool XF = false>
__global__ __launch_bounds__(64 * NW, NW == 16 ? 4 : 2) void k_flux64(FluxArgs a) {
  static_assert(!XF || (RHS && CORR == 1 && sizeof(T) == 8 && R == 2 && XW == 4 && (NW == 4 || NW == 8)), "x-forward transform in the stage kernel: 256-wide rows, fp64");
  static_assert(!RHS || (FUSE && CORR <= 1 && !SKEL && !EXTRA), "right-hand side in the stage kernel: fused epilogue, periodic box, no extra terms");
  static_assert(!CARRY || (FUSE && CORR == 1 && !SKEL && !EXTRA && NW <= 8 && sizeof(T) == 8), "carried combination: the fp64 periodic correcting stage kernel");
  constexpr unsigned EB = (unsigned)sizeof(T);  // element bytes
  const T* const a_u = static_cast<const T*>(a.u);
  const T* const a_pI = static_cast<const T*>(a.pI);
  T* const a_F = static_cast<T*>(a.F);
  static_assert(R + 2 + (CORR ? 1 : 0) <= 8, "packed halo rows live in 8-lane groups");
  int txi, tyi, tzi;
  {
    const int nty_local = (a.nty + 7) >> 3;
    int seq = (int)(blockIdx.x >> 3);
    if (seq >= a.ntx * nty_local * a.ntz) return;
    txi = seq % a.ntx;
    seq /= a.ntx;
    tyi = (int)(blockIdx.x & 7) * nty_local + seq % nty_local;
    tzi = seq / nty_local;
    if (tyi >= a.nty) return;
  }
  __shared__ T rhs_lds_s[RHS ? 2 * NW * R : 1];  // RHS: u* of lane 63, [plane parity][wavefront][row]
  T* const rhs_lds = rhs_lds_s;
  constexpr int XSLOT = (NW / 4) * 256;                   // XF: one plane's rows of a workgroup, 256 complex each
  __shared__ __align__(16) Xc xf_x1[XF ? 2 * XSLOT : 1];  // XF: z, [plane parity][wavefront row][column]
  __shared__ __align__(16) Xc xf_x2[XF ? 2 * XSLOT : 1];  // XF: the transform, [plane parity][wavefront row][fft_swz(position)]
  __shared__ __align__(16) Xc xf_tw[XF ? 6 * 64 : 1];     // XF: per-lane twiddles: [wx][lane] of the first stage, [lane] of the stages Q = 16 and Q = 4
  const int lane = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int wx = wave % XW, wy = wave / XW;
  const int N0 = a.N0, N1 = a.N1, N2 = a.N2;
  const int n0 = N0 - 2, n1 = N1 - 2, n2 = N2 - 2;
  const int x0 = (txi * XW + wx) * 64;  // interior (0-based) column of lane 0
  const int jb0 = (tyi * (NW / XW) + wy) * R;  // interior row of the first output row
  const int k0 = a.kB ? (tzi ? a.kB : a.k_lo) : a.k_lo + tzi * a.zc;  // padded plane index of the first output plane
  const int k1 = a.kB ? k0 + a.zc : min(k0 + a.zc, a.k_hi);
  const int kw0 = RHS ? k0 - 1 : k0;  // first plane of the march
  if (x0 >= n0 || jb0 >= n1) {  // wavefront outside the box: it only keeps the workgroup's barrier count (one per plane)
    if (a.bar || RHS)
      for (int k = kw0; k < k1 + (XF ? 2 : 0); ++k) __builtin_amdgcn_s_barrier();  // (XF: and one per drain iteration)
    return;
  }
  const long long sz = (long long)N0 * N1;
  const int ci = x0 + lane;
  const bool xout = ci < n0;
  const DirT<T> X(a.X), Y(a.Y), Z(a.Z);

  // padded row / column of a (possibly out-of-range) interior index
  auto prow_of = [&](int jr) { return CORR ? wrapi(jr, n1) + 1 : min(jr + 1, N1 - 1); };
  auto pcol_of = [&](int c) { return CORR ? wrapi(c, n0) + 1 : min(c + 1, N0 - 1); };

  // ---- wave-uniform row starts (elements inside a plane) and per-lane byte offsets --------------------------------------
  unsigned urow[R + 2];  // u: byte offset of the padded row inside a plane
  unsigned qrow[R + 3];  // p: byte offset of the interior row inside an unpadded plane (CORR)
#pragma unroll
  for (int rr = 0; rr < R + 2; ++rr) urow[rr] = (unsigned)(prow_of(jb0 - 1 + rr) * N0) * EB;
  if (CORR) {
#pragma unroll
    for (int rr = 0; rr < R + 3; ++rr) qrow[rr] = (unsigned)((prow_of(jb0 - 1 + rr) - 1) * n0) * EB;
  }
  const unsigned ubytes = (unsigned)sz * EB, qbytes = (unsigned)(n0 * n1) * EB;
  // RHS: rows jb0-2 (stencil input, pressure) and jb0-1 (epilogue terms) through the periodic image
  const unsigned urowm2 = (unsigned)((wrapi(jb0 - 2, n1) + 1) * N0) * EB, qrowm2 = (unsigned)(wrapi(jb0 - 2, n1) * n0) * EB;
  const unsigned orowm1 = (unsigned)((wrapi(jb0 - 1, n1) + 1) * N0) * EB;
  const unsigned ucol = (unsigned)pcol_of(ci) * EB;            // main lanes: own column
  const unsigned qcol = CORR ? (unsigned)(pcol_of(ci) - 1) * EB : 0u;
  unsigned uhoff, qhoff = 0;  // packed halo loads: in-plane byte offset of this lane's (row, column)
  {
    const int r = lane & 7, grp = (lane >> 3) & 3;
    const int ru = r <= R + 1 ? r : 0;
    const int colu = (grp == 2) ? pcol_of(x0 + 64) : ((EXTRA && grp == 1) ? pcol_of(x0 - 2) : pcol_of(x0 - 1));  // EXTRA: lanes 8..15 hold column x0-2
    uhoff = (unsigned)(prow_of(jb0 - 1 + ru) * N0 + colu) * EB;
    if (CORR) {
      const int rq = r <= R + 2 ? r : 0;
      const int cq = grp == 0 ? x0 - 1 : (grp == 1 ? x0 : (grp == 2 ? x0 + 64 : x0 + 65));
      qhoff = (unsigned)((prow_of(jb0 - 1 + rq) - 1) * n0 + (pcol_of(cq) - 1)) * EB;
    }
  }

  auto uplane = [&](int kk) {  // padded plane index -> plane actually read
    return CORR == 1 ? wrapi(kk - 1, n2) + 1 : (CORR == 2 ? min(kk, N2 - 1) : ((RHS && kk < 0) ? kk + n2 : kk));
  };
  auto load_plane = [&](Plane<T, R>& P, int kk) {
    const T* base = a_u + (long long)uplane(kk) * sz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const rsrc_t rs = plane_rsrc(base + c * a.sc, ubytes);
#pragma unroll
      for (int rr = 0; rr < R + 2; ++rr) P.v[c][rr] = ldb<T>(rs, ucol, urow[rr]);
      P.h[c] = ldb<T>(rs, uhoff, 0);
      if (RHS && c == 1) P.vm2 = ldb<T>(rs, ucol, urowm2);
    }
  };
  const unsigned urowm1 = (unsigned)(prow_of(jb0 - 2) * N0) * EB;
  auto load_text = [&](TExt<T, R>& E, int kk) {
    const long long po = (long long)uplane(kk) * sz;
    const rsrc_t rt = plane_rsrc(static_cast<const T*>((const void*)a.te.temp) + po, ubytes);
#pragma unroll
    for (int rr = 0; rr < R + 2; ++rr) E.t[rr] = ldb<T>(rt, ucol, urow[rr]);
    E.th = ldb<T>(rt, uhoff, 0);
    E.vm1 = ldb<T>(plane_rsrc(a_u + po + a.sc, ubytes), ucol, urowm1);
  };
  constexpr int NPR = R + 3 + (RHS ? 1 : 0);  // pressure rows jb0-1 .. jb0+R+1; RHS: row jb0-2 behind them
  auto load_p = [&](T (&P)[NPR], T& PH, int kk) {
    const rsrc_t rs = plane_rsrc(a_pI + (long long)(CORR == 2 ? min(kk, N2) : wrapi(kk - 1, n2)) * n0 * n1, qbytes);
#pragma unroll
    for (int rr = 0; rr < R + 3; ++rr) P[rr] = ldb<T>(rs, qcol, qrow[rr]);
    PH = ldb<T>(rs, qhoff, 0);
    if constexpr (RHS) P[R + 3] = ldb<T>(rs, qcol, qrowm2);
  };
  // u = u* - ∇p (applypressure!, operators.jl:225-233) for one register plane and its packed halo columns
  auto correct = [&](Plane<T, R>& P, const T (&Pc)[NPR], T PHc, const T (&Pn)[NPR], T PHn) {
    if (CARRY || a.epi.self_in != 0.0) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) P.raw[c][rr] = P.v[c][rr + 1];
      if constexpr (RHS) P.rawv0 = P.v[1][0];
    }
    if constexpr (RHS) P.vm2 -= (Pc[0] - Pc[R + 3]) * Y.gs;
#pragma unroll
    for (int rr = 0; rr < R + 2; ++rr) {
      const T pc = Pc[rr];
      P.v[0][rr] -= (next_h(pc, rdlane(PHc, 16 + rr)) - pc) * X.gs;
      P.v[1][rr] -= (Pc[rr + 1] - pc) * Y.gs;
      P.v[2][rr] -= (Pn[rr] - pc) * Z.gs;
    }
    P.h[0] -= (dpp_old<0x108>(PHc, PHc) - PHc) * X.gs;  // row_shl:8 — p of the next column, same row
    P.h[1] -= (dpp_old<0x101>(PHc, PHc) - PHc) * Y.gs;  // row_shl:1 — p of the next row, same column
    P.h[2] -= (PHn - PHc) * Z.gs;
  };

  T zprev[3][R];
  T zprevV0 = 0;    // RHS: the same for the y-component at row jb0-1
  T wsprev[R] = {};  // RHS: w* of plane k-1 at the output rows
  auto zflux0 = [&](const Plane<T, R>& C, const Plane<T, R>& Nx) {  // upper-face z-fluxes of the plane below the chunk
    if constexpr (RHS) zprevV0 = flux(C.v[1][0], Nx.v[1][0], C.v[2][0], C.v[2][1], Z.vo);
#pragma unroll
    for (int rr = 1; rr <= R; ++rr) {
      const T Wc = C.v[2][rr];
      zprev[0][rr - 1] = flux(C.v[0][rr], Nx.v[0][rr], Wc, next_h(Wc, rdlane(C.h[2], 16 + rr)), Z.vo);
      zprev[1][rr - 1] = flux(C.v[1][rr], Nx.v[1][rr], Wc, C.v[2][rr + 1], Z.vo);
      zprev[2][rr - 1] = flux(Wc, Nx.v[2][rr], Wc, Nx.v[2][rr], Z.vs);
    }
  };

  // output rows of this wavefront (clamped: rows / columns past the box are computed but never stored)
  unsigned orow[R];
#pragma unroll
  for (int rr = 0; rr < R; ++rr) orow[rr] = (unsigned)((min(jb0 + rr, n1 - 1) + 1) * N0) * EB;
  const unsigned ocol = (unsigned)(min(ci, n0 - 1) + 1) * EB;

  // RK epilogue, first half: s = ustart + Σ_q coef_q k_q for all R rows of plane k.  Issued at the top of the plane so the
  // loads fly during the flux arithmetic (they used to sit right before the stores: one exposed round trip per row).
  T eacc[3][EXTRA ? R : 1];
  T gacc[EXTRA ? R : 1];  // gravity!: α2 avg(temp) at the gdir-face (operators.jl:914-931; uniform grid: the plain mean)
  T Pz[3][EXTRA ? R : 1];  // the output rows of plane k-1 (for the Laplacian behind epi.wout)
  const T nux = X.vs * X.rs, nuy = Y.vs * Y.rs, nuz = Z.vs * Z.rs;  // ν/Δ² per direction (4ν/Δ · ¼/Δ: exact scalings)
  T sV0 = 0;  // RHS: the y-component of s at row jb0-1
  auto epi_load = [&](const Plane<T, R>& C, int k, T (&sacc)[3][R]) {
    const long long pk = (long long)((RHS && k < 1) ? k + n2 : k) * sz;  // (RHS: the plane below the first chunk through its periodic image)
    if constexpr (EXTRA) {
      if (a.epi.extra) {
        const T* b = static_cast<const T*>((const void*)a.epi.extra) + pk;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const rsrc_t rs = plane_rsrc(b + c * a.sc, ubytes);
#pragma unroll
          for (int rr = 0; rr < R; ++rr) eacc[c][rr] = ldb<T>(rs, ocol, orow[rr]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int rr = 0; rr < R; ++rr) eacc[c][rr] = 0;
      }
      if (a.epi.gtemp) {  // temp is a padded scalar field with valid ghost volumes (apply_bc_temp! has run)
        const T* tb = static_cast<const T*>((const void*)a.epi.gtemp) + pk;
        const int gd = a.epi.gdir;
        const rsrc_t r0 = plane_rsrc(tb, ubytes), r1 = plane_rsrc(gd == 2 ? tb + sz : tb, ubytes);
        const unsigned dcol = gd == 0 ? EB : 0u, drow = gd == 1 ? (unsigned)N0 * EB : 0u;
#pragma unroll
        for (int rr = 0; rr < R; ++rr) gacc[rr] = (T)a.epi.ga2 * ((T)0.5 * (ldb<T>(r0, ocol, orow[rr]) + ldb<T>(r1, ocol + dcol, orow[rr] + drow)));
      }
    }
    const bool ntl = (a.nt & 8) != 0;  // INS_FLUX64_NT bit 3: non-temporal loads of the epilogue terms (read once; they share L2 with the re-read velocity planes)
    if (a.epi.ustart) {
      const T* b = static_cast<const T*>((const void*)a.epi.ustart) + pk;
      const T c0 = (T)(1.0 + a.epi.c0m1);  // exactly 1 in the k-basis
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const rsrc_t rs = plane_rsrc(b + c * a.sc, ubytes);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) sacc[c][rr] = c0 * (ntl ? ldb_aux<2>(rs, ocol, orow[rr], (T)0) : ldb<T>(rs, ocol, orow[rr]));
        if (RHS && c == 1) sV0 = c0 * ldb<T>(rs, ocol, orowm1);
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) sacc[c][rr] = C.v[c][rr + 1];
      if constexpr (RHS) sV0 = C.v[1][0];
    }
    if (a.epi.self_in != 0.0) {  // the stencil input is itself a term: no second trip to memory for it
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) sacc[c][rr] += (T)a.epi.self_in * (CORR ? C.raw[c][rr] : C.v[c][rr + 1]);
      if constexpr (RHS) sV0 += (T)a.epi.self_in * (CORR ? C.rawv0 : C.v[1][0]);
    }
    for (int q = 0; q < a.epi.n; ++q) {
      const T* kq = static_cast<const T*>((const void*)a.epi.k[q]) + pk;
      const T cq = (T)a.epi.coef[q];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const rsrc_t rs = plane_rsrc(kq + c * a.sc, ubytes);
        T kv[R];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) kv[rr] = ntl ? ldb_aux<2>(rs, ocol, orow[rr], (T)0) : ldb<T>(rs, ocol, orow[rr]);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) sacc[c][rr] += cq * kv[rr];
        if (RHS && c == 1) sV0 += cq * ldb<T>(rs, ocol, orowm1);
      }
    }
  };
  // second half: u* = s + coef_self f, and k_i = f when a later stage needs it
  // the three components of one result (INS_FLUX64_NT: cache-policy bits on these stores, an experiment)
  auto st3 = [&](T* o, unsigned co, unsigned rowb, T v0, T v1, T v2) {
    const rsrc_t r0 = plane_rsrc(o, ubytes), r1 = plane_rsrc(o + a.sc, ubytes), r2 = plane_rsrc(o + 2 * a.sc, ubytes);
    const int snt = a.nt & 7;
    if (snt == 0) {
      stb(r0, co, rowb, v0);
      stb(r1, co, rowb, v1);
      stb(r2, co, rowb, v2);
    } else if (snt == 1) {
      stb_aux<2>(r0, co, rowb, v0);
      stb_aux<2>(r1, co, rowb, v1);
      stb_aux<2>(r2, co, rowb, v2);
    } else if (snt == 2) {
      stb_aux<17>(r0, co, rowb, v0);
      stb_aux<17>(r1, co, rowb, v1);
      stb_aux<17>(r2, co, rowb, v2);
    } else {
      stb_aux<19>(r0, co, rowb, v0);
      stb_aux<19>(r1, co, rowb, v1);
      stb_aux<19>(r2, co, rowb, v2);
    }
  };
  auto emit = [&](int rr, int k, T fu, T fv, T fw, T s0, T s1, T s2, bool st) {
    const long long pk = (long long)k * sz;
    if constexpr (EXTRA) {
      fu += eacc[0][rr - 1];
      fv += eacc[1][rr - 1];
      fw += eacc[2][rr - 1];
      if (a.epi.gtemp) {
        const T gv = gacc[rr - 1];
        if (a.epi.gdir == 0) fu += gv;
        if (a.epi.gdir == 1) fv += gv;
        if (a.epi.gdir == 2) fw += gv;
      }
    }
    const int j = jb0 + rr - 1;  // interior row
    if (xout && j < n1 && st) {
      const unsigned rowb = orow[rr - 1], co = ocol;
      if (FUSE) {
        if (CORR && a.epi.ustart_out) {  // chained steps: s is the corrected stencil input = this step's ustart (no term was added to it)
          T* w = static_cast<T*>((void*)a.epi.ustart_out) + pk;
          stb(plane_rsrc(w, ubytes), co, rowb, s0);
          stb(plane_rsrc(w + a.sc, ubytes), co, rowb, s1);
          stb(plane_rsrc(w + 2 * a.sc, ubytes), co, rowb, s2);
        }
        T* o = static_cast<T*>((void*)a.epi.ustar) + pk;
        st3(o, co, rowb, s0 + (T)a.epi.coef_self * fu, s1 + (T)a.epi.coef_self * fv, s2 + (T)a.epi.coef_self * fw);
      }
      if (!FUSE || a.epi.write_k) st3(a_F + pk, co, rowb, fu, fv, fw);
    }
  };

  // XF: one iteration of the lagging transform (steps A, B, C above), behind the barrier of iteration k; z = this wavefront's point of plane k
  const int xf_row = wy * 256;
  if constexpr (XF) {
    const Xc* twg = static_cast<const Xc*>((const void*)a.epi.spec_tw);
    auto pw = [](Xc w1, int m) {  // w^m as fft_dif forms it
      const Xc w2 = xc_mul(w1, w1), w3 = xc_mul(w2, w1);
      return m == 0 ? Xc{1.0, 0.0} : (m == 1 ? w1 : (m == 2 ? w2 : w3));
    };
    xf_tw[wx * 64 + lane] = pw(twg[lane], wx);                           // L = 256: W_256^(lane m), m = wx
    xf_tw[256 + lane] = pw(twg[4 * (lane & 15)], lane >> 4);             // L = 64:  W_64^(j m), j = lane % 16, m = lane / 16
    xf_tw[320 + lane] = pw(twg[16 * (lane & 3)], (lane >> 2) & 3);       // L = 16:  W_16^(j m), j = lane % 4, m = (lane / 4) % 4
  }
  auto xf_step = [&](int k, T z0, T z1) {
    if constexpr (XF) {
      int ln = lane;
      asm volatile("" : "+v"(ln));
      if (k >= k0 && k < k1) xf_x1[(k & 1) * XSLOT + xf_row + 64 * wx + ln] = Xc{z0, z1};
      if (k - 1 >= k0 && k - 1 < k1) {
        const Xc* x = xf_x1 + ((k - 1) & 1) * XSLOT + xf_row;
        Xc y = xc_bfly(x[ln], x[ln + 64], x[ln + 128], x[ln + 192], wx);
        if (wx) y = xc_mul(y, xf_tw[wx * 64 + ln]);
        // (ln: the lane index behind a compiler barrier, so that the dozen LDS addresses derived from it are formed here, per plane, and hold no registers across the march)
        Xc* zb = xf_x2 + ((k - 1) & 1) * XSLOT + xf_row + 64 * wx;  // this wavefront's quarter; only the last stage's output is stored rotated
        zb[ln] = y;
        xf_wave_sync();
        {  // Q = 16
          const Xc* e = zb + (ln & 15);
          y = xc_bfly(e[0], e[16], e[32], e[48], ln >> 4);
          y = xc_mul(y, xf_tw[256 + ln]);
          zb[ln] = y;
        }
        xf_wave_sync();
        {  // Q = 4
          const Xc* e = zb + (ln & ~12);
          y = xc_bfly(e[0], e[4], e[8], e[12], (ln >> 2) & 3);
          y = xc_mul(y, xf_tw[320 + ln]);
          zb[ln] = y;
        }
        xf_wave_sync();
        {  // Q = 1 (every lane has read its four inputs when the wavefront's write is issued, so the rotated position may be another lane's input)
          const Xc* e = zb + (ln & ~3);
          y = xc_bfly(e[0], e[1], e[2], e[3], ln & 3);
          zb[xf_swz(64 * wx + ln) - 64 * wx] = y;
        }
      }
      if (k - 2 >= k0 && k - 2 < k1) {
        // the two real rows of plane k-2 (k_xfwd's expressions): A[s] = (Z[s] + conj Z[N-s]) / 2, B[s] = (Z[s] - conj Z[N-s]) / (2i).  Wavefronts 0, 1 store
        // row jb0 (s = 0 .. 127), wavefronts 2, 3 row jb0+1; the lanes with s = 0 also store s = 128.
        const Xc* zr = xf_x2 + (k & 1) * XSLOT + xf_row;
        const int s = (64 * wx + ln) & 127;
        const bool rowb = wx >= 2;
        const unsigned kxs = (unsigned)a.epi.spec_kxs;
        const rsrc_t rs = plane_rsrc(static_cast<double*>((void*)a.epi.spec_out) + 2LL * (k - 3) * kxs * n1, kxs * (unsigned)n1 * 16u);
        const unsigned soff = (unsigned)(jb0 + (rowb ? 1 : 0)) * kxs * 16u;
        auto sep_store = [&](int sk, int sm) {
          const Xc zk = zr[xf_swz(xf_pos(sk))], zm = zr[xf_swz(xf_pos(sm))];
          const Xc av{0.5 * (zk.x + zm.x), 0.5 * (zk.y - zm.y)}, bv{0.5 * (zk.y + zm.y), -0.5 * (zk.x - zm.x)};
          const Xc o = rowb ? bv : av;
          v4u v;
          v.x = (unsigned)__double2loint(o.x), v.y = (unsigned)__double2hiint(o.x), v.z = (unsigned)__double2loint(o.y), v.w = (unsigned)__double2hiint(o.y);
          __builtin_amdgcn_raw_buffer_store_b128(v, rs, (unsigned)sk * 16u, soff, 0);
        };
        sep_store(s, (256 - s) & 255);
        if (s == 0) sep_store(128, 128);
      }
    }
  };

  // One output plane.  C = plane k, Nx = plane k+1 (both complete, corrected).  As soon as a row of C has been consumed its
  // registers are re-loaded with the same row of plane `kload` (= k+2, the next plane this buffer has to hold), so the
  // prefetch of plane k+2 is in flight during the whole of plane k without a third register plane.
  // temperature stage (EXTRA without in-kernel correction, a.tm): state carried from plane to plane
  constexpr bool TMK = EXTRA && CORR == 0;
  T Tz[TMK ? R : 1];      // T of plane k-1 at the output rows
  T wwprev[TMK ? R : 1];  // w·diffusion(w) of plane k-1 at the output rows (zero below the first plane: operators.jl:793-807 reads a ghost of `diff`)
  T PzV0 = 0;               // v at the halo row of plane k-1
  T hU_prev = 0;            // packed halo columns of u, plane k-1
  // st: store this plane's results (RHS: false for the plane below the chunk, which only sets up the carried w*)
  auto body = [&](Plane<T, R>& C, const Plane<T, R>& Nx, TExt<T, R>& CT, const TExt<T, R>& NT, int k, int kload, bool st_) {
    const bool st = RHS ? st_ : true;
    const T* nb = a_u + (long long)uplane(kload) * sz;
    const rsrc_t n0r = plane_rsrc(nb, ubytes), n1r = plane_rsrc(nb + a.sc, ubytes), n2r = plane_rsrc(nb + 2 * a.sc, ubytes);
    const T ch0 = C.h[0], ch1 = C.h[1], ch2 = C.h[2];
    T sacc[3][R];
    if (FUSE) epi_load(C, k, sacc);
    const bool tm = TMK && a.tm;
    const rsrc_t ntr = plane_rsrc(static_cast<const T*>((const void*)a.te.temp) + (long long)uplane(kload) * sz, ubytes);
    T tacc[TMK ? R : 1];
    const T cth = CT.th;
    if constexpr (TMK) {
      if (tm) {  // temp_out = tempstart + Σ_j coef_j ktemp_j + c_self ktemp_i: the loads fly during the flux arithmetic
        const long long pk = (long long)k * sz;
        const rsrc_t rs0 = plane_rsrc(static_cast<const T*>((const void*)a.te.tempstart) + pk, ubytes);
#pragma unroll
        for (int rr = 0; rr < R; ++rr) tacc[rr] = ldb<T>(rs0, ocol, orow[rr]);
        for (int q = 0; q < a.te.n; ++q) {
          const rsrc_t rq = plane_rsrc(static_cast<const T*>((const void*)a.te.k[q]) + pk, ubytes);
#pragma unroll
          for (int rr = 0; rr < R; ++rr) tacc[rr] += (T)a.te.coef[q] * ldb<T>(rq, ocol, orow[rr]);
        }
      }
    }
    T fyu_o = 0, fyv_o = 0, fyw_o = 0;
    T Uo = 0, Vo = 0, Wo = 0;  // row rr - 1 of this plane (EXTRA: its registers already hold the next plane)
    T To = 0, wv_o = 0;        // T and v·diffusion(v) of row rr - 1
    T us_u[RHS ? R : 1], dvs[RHS ? R : 1], dws[RHS ? R : 1];  // RHS: u* and the y / z differences of v* / w* at the output rows
    T vs_o = 0;                                               // RHS: v* of row rr - 1
    T cvm2 = 0;
    if constexpr (RHS) cvm2 = C.vm2;
#pragma unroll
    for (int rr = 0; rr <= R; ++rr) {
      const T Uc = C.v[0][rr], Vc = C.v[1][rr], Wc = C.v[2][rr];
      if (SKEL) {  // timing experiment: same loads, stores and epilogue, trivial arithmetic (tools/scan_flux64.sh)
        if (rr >= 1) {
          const T fu = Uc + fyu_o + C.v[0][rr + 1] + Nx.v[0][rr] + zprev[0][rr - 1] + ch0;
          const T fv = Vc + fyv_o + C.v[1][rr + 1] + Nx.v[1][rr] + zprev[1][rr - 1] + ch1;
          const T fw = Wc + fyw_o + C.v[2][rr + 1] + Nx.v[2][rr] + zprev[2][rr - 1] + ch2;
          emit(rr, k, fu, fv, fw, FUSE ? sacc[0][rr - 1] : (T)0, FUSE ? sacc[1][rr - 1] : (T)0, FUSE ? sacc[2][rr - 1] : (T)0, st);
        }
        fyu_o = Uc;
        fyv_o = Vc;
        fyw_o = Wc;
        C.v[0][rr] = ldb<T>(n0r, ucol, urow[rr]);
        C.v[1][rr] = ldb<T>(n1r, ucol, urow[rr]);
        C.v[2][rr] = ldb<T>(n2r, ucol, urow[rr]);
        continue;
      }
      const T Vn = next_h(Vc, rdlane(ch1, 16 + rr));
      // y-fluxes through the face between rows rr and rr+1
      const T fyu = flux(Uc, C.v[0][rr + 1], Vc, Vn, Y.vo);
      const T fyv = flux(Vc, C.v[1][rr + 1], Vc, C.v[1][rr + 1], Y.vs);
      const T fyw = flux(Wc, C.v[2][rr + 1], Vc, Nx.v[1][rr], Y.vo);
      if (rr >= 1) {
        const T Un = next_h(Uc, rdlane(ch0, 16 + rr)), Wn = next_h(Wc, rdlane(ch2, 16 + rr));
        const T fxu = flux(Uc, Un, Uc, Un, X.vs);
        const T fxv = flux(Vc, Vn, Uc, C.v[0][rr + 1], X.vo);
        const T fxw = flux(Wc, Wn, Uc, Nx.v[0][rr], X.vo);
        // left-face fluxes of lane 0 from the halo column x0-1 (all other lanes take their left neighbour's right face)
        const T sU = rdlane(ch0, rr), sV = rdlane(ch1, rr), sW = rdlane(ch2, rr);
        const T sUu = rdlane(ch0, rr + 1), sUn = rdlane(Nx.h[0], rr);
        const T lxu = flux(sU, Uc, sU, Uc, X.vs);
        const T lxv = flux(sV, Vc, sU, sUu, X.vo);
        const T lxw = flux(sW, Wc, sU, sUn, X.vo);
        T fu = (fxu - prev_h(fxu, lxu)) * X.rs;
        T fv = (fxv - prev_h(fxv, lxv)) * X.ro;
        T fw = (fxw - prev_h(fxw, lxw)) * X.ro;
        fu += (fyu - fyu_o) * Y.ro;
        fv += (fyv - fyv_o) * Y.rs;
        fw += (fyw - fyw_o) * Y.ro;
        const T zu = flux(Uc, Nx.v[0][rr], Wc, Wn, Z.vo);
        const T zv = flux(Vc, Nx.v[1][rr], Wc, C.v[2][rr + 1], Z.vo);
        const T zw = flux(Wc, Nx.v[2][rr], Wc, Nx.v[2][rr], Z.vs);
        fu += (zu - zprev[0][rr - 1]) * Z.ro;
        fv += (zv - zprev[1][rr - 1]) * Z.ro;
        fw += (zw - zprev[2][rr - 1]) * Z.rs;
        zprev[0][rr - 1] = zu;
        zprev[1][rr - 1] = zv;
        zprev[2][rr - 1] = zw;
        if constexpr (EXTRA) {
          // w_α = u_α · diffusion(u)_α at this volume (dissipation!, operators.jl:791-797): the seven-point Laplacian from values already in
          // registers (x: wave shifts, y: the rows above / below, z: plane k+1 and the saved plane k-1)
          if (a.epi.wout || tm) {
            const T Up = prev_h(Uc, sU), Vp = prev_h(Vc, sV), Wp = prev_h(Wc, sW);
            const T wu = Uc * ((Un + Up - 2 * Uc) * nux + (C.v[0][rr + 1] + Uo - 2 * Uc) * nuy + (Nx.v[0][rr] + Pz[0][rr - 1] - 2 * Uc) * nuz);
            const T wv = Vc * ((Vn + Vp - 2 * Vc) * nux + (C.v[1][rr + 1] + Vo - 2 * Vc) * nuy + (Nx.v[1][rr] + Pz[1][rr - 1] - 2 * Vc) * nuz);
            const T ww = Wc * ((Wn + Wp - 2 * Wc) * nux + (C.v[2][rr + 1] + Wo - 2 * Wc) * nuy + (Nx.v[2][rr] + Pz[2][rr - 1] - 2 * Wc) * nuz);
            const int j = jb0 + rr - 1;
            if (a.epi.wout && xout && j < n1) {
              T* w = static_cast<T*>((void*)a.epi.wout) + (long long)k * sz;
              stb(plane_rsrc(w, ubytes), ocol, orow[rr - 1], wu);
              stb(plane_rsrc(w + a.sc, ubytes), ocol, orow[rr - 1], wv);
              stb(plane_rsrc(w + 2 * a.sc, ubytes), ocol, orow[rr - 1], ww);
            }
            if constexpr (TMK) if (tm) {
              // ---- temperature stage at this volume.  Lower-face terms of dissipation!: the left neighbour's w_x by a wave shift — lane 0
              // takes it from the halo column x0-1, whose Laplacian is formed from wave-uniform values (columns x0-2, x0-1 of the packed
              // halo, lane 0's own column, the halo columns of planes k±1) —, the row below from the previous iteration, the plane below
              // from the previous plane; all of them zero below the first volume of a direction (a ghost volume of `diff`).
              T wuL = 0;
              if (x0 > 0) {
                const T U0 = rdlane(Uc, 0), Um2 = rdlane(ch0, 8 + rr), sUd = rdlane(ch0, rr - 1), sUp = rdlane(hU_prev, rr);
                wuL = sU * ((U0 + Um2 - 2 * sU) * nux + (sUu + sUd - 2 * sU) * nuy + (sUn + sUp - 2 * sU) * nuz);
              }
              const T dc = (T)a.te.dcoef;
              const T dd = dc * (prev_h(wu, wuL) + wu) / 2 + dc * (wv_o + wv) / 2 + dc * (wwprev[rr - 1] + ww) / 2;
              // convection_diffusion_temp! (operators.jl:723-737) on the uniform grid: avg = mean, Δ = Δu
              const T Tc = CT.t[rr];
              const T Txp = next_h(Tc, rdlane(cth, 16 + rr)), Txm = prev_h(Tc, rdlane(cth, rr));
              const T Typ = CT.t[rr + 1], Tym = To, Tzp = NT.t[rr], Tzm = Tz[rr - 1];
              const T a4 = (T)a.te.a4;
              T cd = (-(Uc * ((Tc + Txp) / 2) - Up * ((Txm + Tc) / 2)) + a4 * ((Txp - Tc) * X.gs - (Tc - Txm) * X.gs)) * X.gs;
              cd += (-(Vc * ((Tc + Typ) / 2) - Vo * ((Tym + Tc) / 2)) + a4 * ((Typ - Tc) * Y.gs - (Tc - Tym) * Y.gs)) * Y.gs;
              cd += (-(Wc * ((Tc + Tzp) / 2) - Pz[2][rr - 1] * ((Tzm + Tc) / 2)) + a4 * ((Tzp - Tc) * Z.gs - (Tc - Tzm) * Z.gs)) * Z.gs;
              const T kt = cd + dd;
              if (xout && j < n1) {
                const long long pk = (long long)k * sz;
                if (a.te.ktemp_out) stb(plane_rsrc(static_cast<T*>((void*)a.te.ktemp_out) + pk, ubytes), ocol, orow[rr - 1], kt);
                stb(plane_rsrc(static_cast<T*>((void*)a.te.temp_out) + pk, ubytes), ocol, orow[rr - 1], tacc[rr - 1] + (T)a.te.c_self * kt);
              }
              wv_o = wv;
              wwprev[rr - 1] = ww;
              Tz[rr - 1] = Tc;
            }
          }
          Pz[0][rr - 1] = Uc;
          Pz[1][rr - 1] = Vc;
          Pz[2][rr - 1] = Wc;
        }
        emit(rr, k, fu, fv, fw, FUSE ? sacc[0][rr - 1] : (T)0, FUSE ? sacc[1][rr - 1] : (T)0, FUSE ? sacc[2][rr - 1] : (T)0, st);
        if constexpr (CARRY) {  // S at the cells of u* (the predicate and addressing of emit), with the result stores' cache policy: read once, two stages on
          if (xout && jb0 + rr - 1 < n1 && st) {
            const T ca0 = (T)a.epi.ca[0], ca1 = (T)a.epi.ca[1], ca2 = (T)a.epi.ca[2], cs = (T)a.epi.coef_self;
            const T s0 = sacc[0][rr - 1], s1 = sacc[1][rr - 1], s2 = sacc[2][rr - 1];
            st3(static_cast<T*>((void*)a.epi.carry_out) + (long long)k * sz, ocol, orow[rr - 1], ca0 * s0 + ca1 * C.raw[0][rr - 1] + ca2 * (s0 + cs * fu),
                ca0 * s1 + ca1 * C.raw[1][rr - 1] + ca2 * (s1 + cs * fv), ca0 * s2 + ca1 * C.raw[2][rr - 1] + ca2 * (s2 + cs * fw));
          }
        }
        if constexpr (RHS) {  // the stored values (the expressions of emit)
          const T su = sacc[0][rr - 1] + (T)a.epi.coef_self * fu, sv = sacc[1][rr - 1] + (T)a.epi.coef_self * fv, sw = sacc[2][rr - 1] + (T)a.epi.coef_self * fw;
          us_u[rr - 1] = su;
          dvs[rr - 1] = sv - vs_o;
          dws[rr - 1] = sw - wsprev[rr - 1];
          vs_o = sv;
          wsprev[rr - 1] = sw;
          if (lane == 63) rhs_lds[((k & 1) * NW + wave) * R + rr - 1] = su;
        }
      } else if constexpr (RHS) {
        // v* at row jb0-1: the y-component of the rr >= 1 branch, term by term.  (A lambda shared by both rows was tried: it moved the register allocation of every
        // existing instantiation, +4 VGPRs and one wave per SIMD less in the non-correcting 2-row kernels; the rhs test of tests/test_gpu_stage_rhs.py, which
        // observes a bitwise-equal result today, pins the two copies together.)
        const T fyv_m = flux(cvm2, Vc, cvm2, Vc, Y.vs);
        const T fxv = flux(Vc, Vn, Uc, C.v[0][rr + 1], X.vo);
        const T lxv = flux(rdlane(ch1, rr), Vc, rdlane(ch0, rr), rdlane(ch0, rr + 1), X.vo);
        T fv = (fxv - prev_h(fxv, lxv)) * X.ro;
        fv += (fyv - fyv_m) * Y.rs;
        const T zv = flux(Vc, Nx.v[1][rr], Wc, C.v[2][rr + 1], Z.vo);
        fv += (zv - zprevV0) * Z.ro;
        zprevV0 = zv;
        vs_o = sV0 + (T)a.epi.coef_self * fv;
      }
      fyu_o = fyu;
      fyv_o = fyv;
      fyw_o = fyw;
      if constexpr (TMK) {
        if (tm) {
          if (rr == 0) {  // v·diffusion(v) at the halo row (the row below the first output row; a ghost row of `diff` when it is row -1 of the box)
            const T Vp = prev_h(Vc, rdlane(ch1, 0));
            wv_o = jb0 > 0 ? Vc * ((Vn + Vp - 2 * Vc) * nux + (C.v[1][1] + CT.vm1 - 2 * Vc) * nuy + (Nx.v[1][0] + PzV0 - 2 * Vc) * nuz) : (T)0;
            PzV0 = Vc;
          }
          To = CT.t[rr];
          CT.t[rr] = ldb<T>(ntr, ucol, urow[rr]);
        }
      }
      if constexpr (EXTRA) {
        Uo = Uc;
        Vo = Vc;
        Wo = Wc;
      }
      // row rr of plane k is dead: its registers receive plane `kload`
      C.v[0][rr] = ldb<T>(n0r, ucol, urow[rr]);
      C.v[1][rr] = ldb<T>(n1r, ucol, urow[rr]);
      C.v[2][rr] = ldb<T>(n2r, ucol, urow[rr]);
    }
    C.v[0][R + 1] = ldb<T>(n0r, ucol, urow[R + 1]);
    C.v[1][R + 1] = ldb<T>(n1r, ucol, urow[R + 1]);
    C.v[2][R + 1] = ldb<T>(n2r, ucol, urow[R + 1]);
    C.h[0] = ldb<T>(n0r, uhoff, 0);
    C.h[1] = ldb<T>(n1r, uhoff, 0);
    C.h[2] = ldb<T>(n2r, uhoff, 0);
    if constexpr (RHS) {
      C.vm2 = ldb<T>(n1r, ucol, urowm2);
      // every wavefront's lane-63 u* of this plane is in LDS behind the barrier; the slot is written again two planes on, behind the next barrier, when every
      // wavefront has read it.  Fences on LDS only: a fence on global memory would wait for the prefetch of plane k+2.
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      const int lw = wy * XW + (wx + XW - 1) % XW;
      T* ro = static_cast<T*>((void*)a.epi.rhs_out) + (long long)(k - 1) * n0 * n1;
      const rsrc_t rr_ = plane_rsrc(ro, qbytes);
      const T om = (T)a.om;
      T zz[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const T ul = rhs_lds[((k & 1) * NW + lw) * R + r];
        T d = 0;  // Ω·div(u*): the expression of k_xfwd<XSRC_DIV> (ins_fft.hip)
        d += (us_u[r] - prev_h(us_u[r], ul)) * (T)a.rdiv[0];
        d += dvs[r] * (T)a.rdiv[1];
        d += dws[r] * (T)a.rdiv[2];
        zz[r] = d * om;
        if (!XF && st && xout && jb0 + r < n1) stb(rr_, (unsigned)min(ci, n0 - 1) * EB, (unsigned)(min(jb0 + r, n1 - 1) * n0) * EB, zz[r]);
      }
      if constexpr (XF) xf_step(k, zz[0], zz[1]);  // (st == (k >= k0): the plane below the chunk enters nothing)
    }
    if constexpr (TMK) {
      if (tm) {
        hU_prev = ch0;
        CT.t[R + 1] = ldb<T>(ntr, ucol, urow[R + 1]);
        CT.th = ldb<T>(ntr, uhoff, 0);
        CT.vm1 = ldb<T>(n1r, ucol, urowm1);
      }
    }
  };

  // Two register planes.  Loads past the chunk re-read plane k1 / p(k1+1) (cache hits) instead of branching.
  Plane<T, R> P0, P1;
  TExt<T, R> TE0, TE1;
  if (!CORR) {
    load_plane(P0, kw0 - 1);
    load_plane(P1, kw0);
    zflux0(P0, P1);
    if constexpr (EXTRA) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) Pz[c][rr] = P0.v[c][rr + 1];
      if (a.tm) {
        load_text(TE0, k0 - 1);
        load_text(TE1, k0);
        PzV0 = P0.v[1][0];
        hU_prev = P0.h[0];
        // w·diffusion(w) of plane k0-1 (zero when that is the ghost plane): its z-neighbour below, plane k0-2, is read here once per chunk
        const rsrc_t rw = plane_rsrc(a_u + (long long)uplane(max(k0 - 2, 0)) * sz + 2 * a.sc, ubytes);
#pragma unroll
        for (int rr = 1; rr <= R; ++rr) {
          const T Wc = P0.v[2][rr], Wm2 = ldb<T>(rw, ucol, urow[rr]);
          const T Wn = next_h(Wc, rdlane(P0.h[2], 16 + rr)), Wp = prev_h(Wc, rdlane(P0.h[2], rr));
          wwprev[rr - 1] = k0 > 1 ? Wc * ((Wn + Wp - 2 * Wc) * nux + (P0.v[2][rr + 1] + P0.v[2][rr - 1] - 2 * Wc) * nuy + (P1.v[2][rr] + Wm2 - 2 * Wc) * nuz) : (T)0;
          Tz[rr - 1] = TE0.t[rr];
        }
      }
    }
    load_plane(P0, min(kw0 + 1, k1));
    if constexpr (EXTRA) {
      if (a.tm) load_text(TE0, min(k0 + 1, k1));
    }
    int k = kw0;
    while (true) {
      if (!RHS && a.bar) __builtin_amdgcn_s_barrier();
      body(P1, P0, TE1, TE0, k, min(k + 2, k1), k >= k0);
      if (++k >= k1) break;
      if (!RHS && a.bar) __builtin_amdgcn_s_barrier();
      body(P0, P1, TE0, TE1, k, min(k + 2, k1), k >= k0);
      if (++k >= k1) break;
    }
  } else {
    // invariant at the top of iteration k: cur = corrected plane k, nxt = RAW plane k+1, Pa = p(k+1), Pb = p(k+2)
    T Pa[NPR], Pb[NPR], Ha, Hb;
    load_p(Pa, Ha, kw0 - 1);
    load_p(Pb, Hb, kw0);
    load_plane(P0, kw0 - 1);
    load_plane(P1, kw0);
    correct(P0, Pa, Ha, Pb, Hb);
    load_p(Pa, Ha, kw0 + 1);
    correct(P1, Pb, Hb, Pa, Ha);
    zflux0(P0, P1);
    if constexpr (EXTRA) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int rr = 0; rr < R; ++rr) Pz[c][rr] = P0.v[c][rr + 1];
    }
    load_plane(P0, min(kw0 + 1, k1));
    load_p(Pb, Hb, min(kw0 + 2, k1 + 1));
    int k = kw0;
    while (true) {
      if (!RHS && a.bar) __builtin_amdgcn_s_barrier();
      correct(P0, Pa, Ha, Pb, Hb);  // plane k+1 with p(k+1), p(k+2)
      load_p(Pa, Ha, min(k + 3, k1 + 1));
      body(P1, P0, TE1, TE0, k, min(k + 2, k1), k >= k0);
      if (++k >= k1) break;
      if (!RHS && a.bar) __builtin_amdgcn_s_barrier();
      correct(P1, Pb, Hb, Pa, Ha);
      load_p(Pb, Hb, min(k + 3, k1 + 1));
      body(P0, P1, TE0, TE1, k, min(k + 2, k1), k >= k0);
      if (++k >= k1) break;
    }
    if constexpr (XF) {  // the two planes still in the pipeline
      for (int kd = k1; kd < k1 + 2; ++kd) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        xf_step(kd, (T)0, (T)0);
      }
    }
  }
}

// tile-shape knobs: run-time options (ins_options.hip; environment variable of the same name, or ins_set_option)
#define g_disable ((int)ins_opt(OPT_INS_DISABLE_FLUX64))
#define g_rows ((int)ins_opt(OPT_INS_FLUX64_ROWS))
#define g_rows_corr ((int)ins_opt(OPT_INS_FLUX64_ROWS_CORR))
#define g_zchunk ((int)ins_opt(OPT_INS_FLUX64_ZC))
#define g_zchunk_corr ((int)ins_opt(OPT_INS_FLUX64_ZC_CORR))
#define g_xw ((int)ins_opt(OPT_INS_FLUX64_XW))
#define g_lds ((int)ins_opt(OPT_INS_FLUX64_LDS))    // experiment: dynamic LDS bytes per workgroup (caps workgroups per CU)
#define g_skel ((int)ins_opt(OPT_INS_FLUX64_SKEL))  // timing experiment only: wrong results by design

template <typename T, int R, int XW, bool FUSE, int NW>
int launch_range(const ins_grid* G, FluxArgs& a, int corr_mode, hipStream_t s) {
  const unsigned nb = (unsigned)(8LL * a.ntx * ((a.nty + 7) / 8) * a.ntz);
  if (nb == 0) return INS_OK;
  const dim3 block(64, NW, 1);
  if constexpr (NW <= 8 && R == 4 && sizeof(T) == 8) {
    if (g_skel && corr_mode == 0) {
      hipLaunchKernelGGL((k_flux64<T, R, XW, FUSE, 0, true, NW>), dim3(nb), block, (size_t)g_lds, s, a);
      INS_LAUNCH_CHECK();
      return INS_OK;
    }
  }
  if (a.tm && corr_mode != 0) {
    ins_set_error("temperature stage inside the stage kernel: no in-kernel pressure correction");
    return INS_ERR_UNSUPPORTED;
  }
  if (a.epi.extra || a.epi.gtemp || a.epi.wout || a.tm) {
    if constexpr (FUSE && R == 2 && NW == 4 && sizeof(T) == 8) {
      if (corr_mode == 0) {
        hipLaunchKernelGGL((k_flux64<T, R, XW, true, 0, false, NW, true>), dim3(nb), block, (size_t)g_lds, s, a);
        INS_LAUNCH_CHECK();
        return INS_OK;
      }
      if (corr_mode == 1) {
        hipLaunchKernelGGL((k_flux64<T, R, XW, true, 1, false, NW, true>), dim3(nb), block, (size_t)g_lds, s, a);
        INS_LAUNCH_CHECK();
        return INS_OK;
      }
    }
    ins_set_error("stage kernel with an extra force term: fp64, fused epilogue, 2 rows, 4 wavefronts, no slab correction");
    return INS_ERR_UNSUPPORTED;
  }
  if (corr_mode == 0)
    hipLaunchKernelGGL((k_flux64<T, R, XW, FUSE, 0, false, NW>), dim3(nb), block, (size_t)g_lds, s, a);
  else if constexpr (FUSE && R <= 5) {
    if (corr_mode == 1 && a.epi.carry_out) {
      if constexpr (R == 2 && NW <= 8 && sizeof(T) == 8) {
        hipLaunchKernelGGL((k_flux64<T, R, XW, true, 1, false, NW, false, false, true>), dim3(nb), block, (size_t)g_lds, s, a);
      } else {
        ins_set_error("stage kernel asked to carry a combination forward on a tile shape it does not do it for");
        return INS_ERR_UNSUPPORTED;
      }
    } else if (corr_mode == 1)
      hipLaunchKernelGGL((k_flux64<T, R, XW, true, 1, false, NW>), dim3(nb), block, (size_t)g_lds, s, a);
    else
      hipLaunchKernelGGL((k_flux64<T, R, XW, true, 2, false, NW>), dim3(nb), block, (size_t)g_lds, s, a);
  } else {
    ins_set_error("in-kernel pressure correction needs the fused epilogue and <= 5 rows per thread");
    return INS_ERR_UNSUPPORTED;
  }
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// part 0: every plane; 1: the planes that read no ghost plane, [1 + ZB, nzl + 1 - ZB); 2: the two boundary ranges of ZB planes
constexpr int ZB = 4;
template <typename T, int R, int XW, bool FUSE, int NW = 4>
int launch(const ins_grid* G, FluxArgs& a, int corr_mode, int part, hipStream_t s) {
  const GridDev& g = G->g;
  a.ntx = cdiv(g.N[0] - 2, 64 * XW);
  a.nty = cdiv(g.N[1] - 2, (NW / XW) * R);
  const int nzl = g.N[2] - 2;
  a.k_lo = 1;
  a.k_hi = nzl + 1;
  a.kB = 0;
  if (part != 0 && nzl <= 2 * ZB) {  // too thin to split: everything in part 2
    if (part == 1) return INS_OK;
    part = 0;
  }
  if (part == 1) {
    a.k_lo = 1 + ZB;
    a.k_hi = nzl + 1 - ZB;
  } else if (part == 2) {
    a.zc = ZB;
    a.kB = nzl + 1 - ZB;
  }
  a.ntz = part == 2 ? 2 : cdiv(a.k_hi - a.k_lo, a.zc);
  return launch_range<T, R, XW, FUSE, NW>(G, a, corr_mode, s);
}

// the instantiations that also write Ω·div(u*) (a.epi.rhs_out): fp64, whole rows per workgroup, every plane in one launch
template <int R, int XW, int NW, int CORR, bool CARRY = false, bool XF = false>
int launch_rhs(const ins_grid* G, FluxArgs& a, hipStream_t s) {
  const GridDev& g = G->g;
  a.ntx = 1;
  a.nty = cdiv(g.N[1] - 2, (NW / XW) * R);
  a.k_lo = 1;
  a.k_hi = g.N[2] - 1;
  a.kB = 0;
  a.ntz = cdiv(a.k_hi - a.k_lo, a.zc);
  const unsigned nb = (unsigned)(8LL * ((a.nty + 7) / 8) * a.ntz);
  hipLaunchKernelGGL((k_flux64<double, R, XW, true, CORR, false, NW, false, true, CARRY, XF>), dim3(nb), dim3(64, NW, 1), 0, s, a);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

}  // namespace

// Tuning knobs for experiments in one process on one allocation (not part of the public ABI); -1 keeps a value.
extern "C" void ins_tune_flux64(int disable, int rows, int rows_corr, int zchunk, int xw, int skel, int burst_unused, int lds) {
  if (disable >= 0) ins_set_option("INS_DISABLE_FLUX64", disable);
  if (rows >= 0) ins_set_option("INS_FLUX64_ROWS", rows);
  if (rows_corr >= 0) ins_set_option("INS_FLUX64_ROWS_CORR", rows_corr);
  if (zchunk >= 0) ins_set_option("INS_FLUX64_ZC", zchunk);
  if (xw >= 0) ins_set_option("INS_FLUX64_XW", xw);
  if (skel >= 0) ins_set_option("INS_FLUX64_SKEL", skel);
  (void)burst_unused;
  if (lds >= 0) ins_set_option("INS_FLUX64_LDS", lds);
}

// 3-D, every interior volume a DOF (all-periodic box or periodic slab), bitwise-constant metric records, room for the
// periodic wrap of a full wavefront window.
bool ins_flux64_supported(const ins_grid* G) {
  const GridDev& g = G->g;
  return !g_disable && g.D == 3 && G->all_dof && G->uniform_exact && g.N[0] - 2 >= 66 && g.N[1] - 2 >= 8 && g.N[2] - 2 >= 4;
}

// Workgroup shape of a launch: xw wavefronts side by side, nw per workgroup, `rows` output rows per lane, z-chunks of zc planes.  A function of the box and of
// the tile-shape options; ext: the extended stage loop's instantiation; rhs: the caller wants the Poisson right-hand side from the kernel.
struct TileShape {
  int xw, rows, nw, zc;
};
static TileShape tile_shape(const ins_grid* G, int corr_mode, bool f32, bool ext, bool rhs) {
  const GridDev& g = G->g;
  const int n2 = g.N[2] - 2;
  const int waves_x = cdiv(g.N[0] - 2, 64);
  // wavefronts side by side: 4 for 256-wide rows (2.85 vs 2.90 ms/step with 2), 2 for 512-wide ones (23.7 vs 24.3 ms/step)
  const int xwo = (corr_mode && ins_opt(OPT_INS_FLUX64_XW_CORR)) ? (int)ins_opt(OPT_INS_FLUX64_XW_CORR) : g_xw;
  int xw = xwo ? xwo : (waves_x >= 8 ? 2 : (waves_x >= 4 ? 4 : (waves_x >= 2 ? 2 : 1)));
  if (!xwo)  // rows of 3 or 6 wavefronts (192, 384 columns): side-by-side counts that leave no wavefront outside the box
    while (xw > 1 && cdiv(waves_x, xw) * xw > waves_x) xw >>= 1;
  // a stage kernel that writes the Poisson right-hand side needs workgroups that span whole rows: 192 columns as three wavefronts side by side, two such rows
  const bool three = rhs && corr_mode == 1 && !xwo && waves_x == 3 && !ins_opt(OPT_INS_FLUX64_NW);
  if (three) xw = 3;
  int rows = corr_mode ? (g_rows_corr ? g_rows_corr : 2) : (g_rows ? g_rows : 4);
  rows = std::min(std::max(rows, 2), corr_mode ? 5 : 6);
  // the fp32 family is built for the default shapes only (2 rows correcting, 4 otherwise)
  if (f32) rows = corr_mode ? (ins_opt(OPT_INS_F32_CORR_ROWS) == 4 ? 4 : 2) : 4;
  // Workgroup shape and z-chunk.  The wavefronts of a workgroup share halo rows / columns; a workgroup barrier per plane keeps them on
  // the same plane, so those shared lines are cache hits instead of HBM re-reads (512^3 plain K1, same box: 1.45 -> 1.37 ms with 4
  // wavefronts, 1.28 ms with 8 wavefronts = 128 x 16 cells per plane and workgroup: the flat-copy rate of that box, profiles/r02_k1_lab.txt;
  // without the barrier 8 wavefronts are SLOWER than 4: 1.53 ms).  Every z-chunk re-reads two planes ((zc+2)/zc), so chunks are as long as
  // the tile count allows: 8 wavefronts and 64-plane chunks when that still gives every CU a workgroup (256^3: the correcting kernel, 2 rows
  // per thread; 512^3: every kernel), else 4 wavefronts (256^3 plain K1: 8 wavefronts x 64 planes would leave half the CUs idle, 0.30 vs
  // 0.205 ms; x 32 planes 0.213 ms).  Same-box steps: 256^3 2.69 (4 wavefronts) -> 2.64 ms, 512^3 23.7 -> 22.35 ms (profiles/r02a_step_lab.txt).
  const int nwo = (int)ins_opt(OPT_INS_FLUX64_NW);
  const int zco = (corr_mode && g_zchunk_corr) ? g_zchunk_corr : g_zchunk;
  auto tiles = [&](int nw_, int zc_) {
    return (long long)cdiv(g.N[0] - 2, 64 * xw) * cdiv(g.N[1] - 2, (nw_ / xw) * rows) * cdiv(n2, zc_);
  };
  const long long mintiles = ins_opt(OPT_INS_FLUX64_MINTILES) > 0 ? ins_opt(OPT_INS_FLUX64_MINTILES) : 256;  // one workgroup per CU
  int nw = three ? 6 : (nwo == 16 ? 16 : (nwo == 8 ? 8 : (nwo == 4 ? 4 : 0)));
  int zc = zco;
  if (!nw) {
    nw = 4;
    if (xw <= 8 && !g_lds) {
      for (int z : {64}) {
        const int zt = zco ? zco : z;
        if (n2 >= zt && tiles(8, zt) >= mintiles) {
          nw = 8;
          zc = zt;
          break;
        }
      }
    }
  }
  if (!zc) {
    const bool small_plane = (long long)(g.N[0] - 2) * (g.N[1] - 2) <= 256LL * 256;
    zc = n2 >= 256 && small_plane ? 64 : (n2 >= 128 ? 32 : (n2 >= 64 ? 16 : (n2 >= 32 ? 8 : 4)));
    // boxes below 256 planes: chunks as long as two workgroups per CU allow (128^3: 32-plane chunks are 128 workgroups for 256 CUs —
    // 0.61 ms/step; 8-plane chunks 0.45)
    if (n2 < 256)
      while (zc > 4 && tiles(nw, zc) < 2 * mintiles) zc >>= 1;
  }
  if (rows != 2 && nw == 16) nw = 8;
  if (ext) {  // one instantiation serves the extended stage loop
    rows = 2;
    nw = 4;
    if (!zco) zc = n2 >= 128 ? 32 : (n2 >= 64 ? 16 : (n2 >= 32 ? 8 : 4));
  }
  return TileShape{xw, rows, nw, zc};
}

// The one place that decides whether a stage kernel launch (fp64, fused epilogue, no extra terms, every plane) writes the Poisson right-hand side: the launch is
// this file's kernel, its workgroups span whole rows (so u*(i-1) never belongs to another workgroup) and the tile shape is one the route is built for.
bool ins_flux64_stage_rhs_supported(const ins_grid* G, int corr_mode) {
  if (ins_opt(OPT_INS_DISABLE_STAGE_RHS) || corr_mode < 0 || corr_mode > 1 || !ins_flux64_supported(G) || g_skel || g_lds) return false;
  if (ins_flux128_supported(G, nullptr, corr_mode, false)) return false;
  const TileShape t = tile_shape(G, corr_mode, false, false, true);
  if (64 * t.xw != G->g.N[0] - 2) return false;
  if (corr_mode == 0) return t.rows == 4 && t.xw == 2 && t.nw == 4;
  return t.rows == 2 && ((t.xw == 3 && t.nw == 6) || ((t.xw == 2 || t.xw == 4) && (t.nw == 4 || t.nw == 8)));
}

// ... and whether it stores the x-spectrum of that right-hand side instead (XF; INS_DISABLE_STAGE_XFWD=1: never): the right-hand-side route holds, the rows are 256
// wide and the tile shape is 2 rows x 4 wavefronts side by side, 4 or 8 wavefronts per workgroup.  The solver's half (own x pass in front of the y pass) is
// ins_poisson_stage_spec_possible's.  128- and 192-wide rows would start with a radix-2 / radix-3 stage across wavefronts: not built, they keep the array.
bool ins_flux64_stage_xfwd_supported(const ins_grid* G, int corr_mode) {
  if (ins_opt(OPT_INS_DISABLE_STAGE_XFWD) || corr_mode != 1 || !ins_flux64_stage_rhs_supported(G, corr_mode)) return false;
  if (G->g.N[0] - 2 != 256 || (G->g.N[1] & 1)) return false;
  const TileShape t = tile_shape(G, corr_mode, false, false, true);
  return t.rows == 2 && t.xw == 4 && (t.nw == 4 || t.nw == 8);
}

// A correcting stage (corr_mode 1, fp64, every plane) can also store a carried combination (RkEpi::carry_out): this file's kernel runs it, in the default 2-row
// shape with 4, 6 or 8 wavefronts (the 16-wavefront form has half the registers).
bool ins_flux64_stage_carry_supported(const ins_grid* G) {
  if (ins_opt(OPT_INS_DISABLE_STAGE_CARRY) || !ins_flux64_supported(G) || g_skel) return false;
  if (ins_flux128_supported(G, nullptr, 1, false)) return false;
  const TileShape t = tile_shape(G, 1, false, false, false);  // (asking for the right-hand side changes xw and nw of 192-wide rows only: 3 and 6)
  return t.rows == 2 && t.nw <= 8;
}

// corr_mode 0: u has valid ghost volumes.  1 / 2: see k_flux64.  fuse: RK epilogue `epi`.
template <typename T>
static int flux64_dispatch(const ins_grid* G, double visc, const T* u, T* F, const RkEpi* epi, const T* pI, int corr_mode, hipStream_t s, int part) {
  const GridDev& g = G->g;
  FluxArgs a;
  memset(&a, 0, sizeof(a));
  a.u = u;
  a.pI = pI;
  a.F = F;
  a.sc = g.sc;
  a.N0 = g.N[0];
  a.N1 = g.N[1];
  a.N2 = g.N[2];
  a.X = make_dir(G, 0, visc);
  a.Y = make_dir(G, 1, visc);
  a.Z = make_dir(G, 2, visc);
  if (epi) a.epi = *epi;
  if (epi && epi->tstage) {
    a.te = *epi->tstage;
    a.tm = 1;
    a.epi.tstage = nullptr;
  }
  const bool ext = epi && (epi->extra || epi->gtemp || epi->wout || epi->tstage);
  const bool want_spec = epi && epi->spec_out;
  const bool want_rhs = epi && (epi->rhs_out || want_spec);
  const TileShape ts = tile_shape(G, corr_mode, sizeof(T) == 4, ext, want_rhs);
  const int xw = ts.xw, rows = ts.rows, nw = ts.nw, zc = ts.zc;
  constexpr bool F32 = sizeof(T) == 4;
  a.zc = zc;
  a.bar = ins_opt(OPT_INS_FLUX64_NOBAR) ? 0 : 1;
  // cache-policy bits of the stage kernel's once-only streams: bit 0 = nt on the result stores, bit 3 = nt on the loads of the epilogue terms (ustart, stage terms).
  // Default: both (256^3 step 2.538 -> 2.518 ms same-box, 512^3 21.09 -> 20.99: the re-read velocity planes keep more of L2); INS_FLUX64_NT=16: plain; 1 / 2 / 3 / 8: the
  // single experiments (profiles/r03_nt_lab.txt)
  {
    const long long o = ins_opt(OPT_INS_FLUX64_NT);
    a.nt = o == 0 ? ((epi && !F32) ? 9 : 0) : (o == 16 ? 0 : (int)o);  // the plain kernel (no epilogue) lost with nt stores in round 1's experiment: stage kernels only; fp32 not measured
  }
#define INS_F64_CASE(RR, FUSE)                                                        \
  if constexpr (!F32 || RR == 2 || RR == 4) {                                         \
    if (rows == RR) {                                                                 \
      if constexpr (RR == 2 && !F32) {                                                \
        if (nw == 16) {                                                               \
          if (xw == 4) return launch<T, RR, 4, FUSE, 16>(G, a, corr_mode, part, s);   \
          if (xw == 2) return launch<T, RR, 2, FUSE, 16>(G, a, corr_mode, part, s);   \
          return launch<T, RR, 1, FUSE, 16>(G, a, corr_mode, part, s);                \
        }                                                                             \
      }                                                                               \
      if (nw >= 8) {                                                                  \
        if (xw == 4) return launch<T, RR, 4, FUSE, 8>(G, a, corr_mode, part, s);      \
        if (xw == 2) return launch<T, RR, 2, FUSE, 8>(G, a, corr_mode, part, s);      \
        return launch<T, RR, 1, FUSE, 8>(G, a, corr_mode, part, s);                   \
      }                                                                               \
      if (xw == 4) return launch<T, RR, 4, FUSE>(G, a, corr_mode, part, s);           \
      if (xw == 2) return launch<T, RR, 2, FUSE>(G, a, corr_mode, part, s);           \
      return launch<T, RR, 1, FUSE>(G, a, corr_mode, part, s);                        \
    }                                                                                 \
  }
  const bool carry = epi && epi->carry_out;
  if (carry) {
    if (ins_stage_carry_aliases(*epi, u) || ins_stage_out_aliases_input(*epi, u)) {  // other workgroups still read the halo rows and planes of the inputs
      ins_set_error("stage kernel asked to carry a combination forward into, or to store u* over, one of its inputs");
      return INS_ERR_INVALID;
    }
    if (F32 || corr_mode != 1 || part != 0 || !ins_flux64_stage_carry_supported(G)) {
      ins_set_error("stage kernel asked to carry a combination forward on a path that does not do it");
      return INS_ERR_UNSUPPORTED;
    }
  }
  if (want_rhs) {
    if (ins_stage_out_aliases_input(*epi, u)) {  // the right-hand side reads neighbouring cells of every input
      ins_set_error("stage kernel asked for the Poisson right-hand side while u* overwrites one of its inputs");
      return INS_ERR_INVALID;
    }
    if (want_spec && (epi->rhs_out || F32 || part != 0 || !ins_flux64_stage_xfwd_supported(G, corr_mode) || !epi->spec_tw || epi->spec_kxs < 129 ||
                      (const void*)epi->spec_out == (const void*)pI)) {
      ins_set_error("stage kernel asked for the x-spectrum of the Poisson right-hand side on a box, tile shape or buffer it does not write it for");
      return INS_ERR_UNSUPPORTED;
    }
    if constexpr (!F32) {
      if (part == 0 && ins_flux64_stage_rhs_supported(G, corr_mode)) {
        a.rdiv[0] = 1.0 / G->desc.dx[0][1];
        a.rdiv[1] = 1.0 / G->desc.dx[1][1];
        a.rdiv[2] = 1.0 / G->desc.dx[2][1];
        a.om = G->desc.dx[0][1] * G->desc.dx[1][1] * G->desc.dx[2][1];
        if (corr_mode == 0) return launch_rhs<4, 2, 4, 0>(G, a, s);
        if (want_spec) {
          if (carry) return nw == 8 ? launch_rhs<2, 4, 8, 1, true, true>(G, a, s) : launch_rhs<2, 4, 4, 1, true, true>(G, a, s);
          return nw == 8 ? launch_rhs<2, 4, 8, 1, false, true>(G, a, s) : launch_rhs<2, 4, 4, 1, false, true>(G, a, s);
        }
        if (carry) {
          if (xw == 3) return launch_rhs<2, 3, 6, 1, true>(G, a, s);
          if (xw == 4) return nw == 8 ? launch_rhs<2, 4, 8, 1, true>(G, a, s) : launch_rhs<2, 4, 4, 1, true>(G, a, s);
          return nw == 8 ? launch_rhs<2, 2, 8, 1, true>(G, a, s) : launch_rhs<2, 2, 4, 1, true>(G, a, s);
        }
        if (xw == 3) return launch_rhs<2, 3, 6, 1>(G, a, s);
        if (xw == 4) return nw == 8 ? launch_rhs<2, 4, 8, 1>(G, a, s) : launch_rhs<2, 4, 4, 1>(G, a, s);
        return nw == 8 ? launch_rhs<2, 2, 8, 1>(G, a, s) : launch_rhs<2, 2, 4, 1>(G, a, s);
      }
    }
    ins_set_error("stage kernel asked for the Poisson right-hand side on a box or tile shape it does not write it for");
    return INS_ERR_UNSUPPORTED;
  }
  if (epi) {
    INS_F64_CASE(2, true)
    INS_F64_CASE(3, true)
    INS_F64_CASE(4, true)
    INS_F64_CASE(5, true)
    INS_F64_CASE(6, true)
  } else {
    INS_F64_CASE(2, false)
    INS_F64_CASE(3, false)
    INS_F64_CASE(4, false)
    INS_F64_CASE(5, false)
    INS_F64_CASE(6, false)
  }
#undef INS_F64_CASE
  return INS_ERR_INVALID;
}

// two x-columns per lane (16 B per lane and memory instruction) wherever the box allows it: ins_flux128.hip
int ins_k_flux64(const ins_grid* G, double visc, const double* u, double* F, const RkEpi* epi, const double* pI, int corr_mode, hipStream_t s,
                 int part) {
  if (ins_flux128_supported(G, epi, corr_mode, false)) {
    if (epi && epi->carry_out) {
      ins_set_error("stage kernel asked to carry a combination forward on a path that does not do it");
      return INS_ERR_UNSUPPORTED;
    }
    return ins_k_flux128(G, visc, u, F, epi, pI, corr_mode, s, part);
  }
  return flux64_dispatch<double>(G, visc, u, F, epi, pI, corr_mode, s, part);
}
// fp32 family (`_f32` entry points): same kernels instantiated for float; RkEpi's pointers are float arrays then
int ins_k_flux64_f32(const ins_grid* G, double visc, const float* u, float* F, const RkEpi* epi, const float* pI, int corr_mode, hipStream_t s,
                     int part) {
  if (ins_flux128_supported(G, epi, corr_mode, true) && !ins_opt(OPT_INS_F32_ONE_COLUMN)) return ins_k_flux128_f32(G, visc, u, F, epi, pI, corr_mode, s, part);
  return flux64_dispatch<float>(G, visc, u, F, epi, pI, corr_mode, s, part);
}
