// Observing an ensemble (ins_rk_ensemble.hip): the blocking diagnostics of a single field — ins_total_kinetic_energy_f64, ins_max_abs_divergence_f64,
// ins_cfl_timestep_f64 (ins_operators.hip) and ins_spectrum_f64 (ins_spectrum.hip) — for all B members of a handle in a launch count that does not depend on B,
// with no allocation per call and no host synchronisation inside an entry.
//   * ins_rk_ensemble_stats_f64: ONE pass over U forms the three per-cell quantities (the text of k_kinetic_energy + k_scalewithvolume, k_divergence and k_cfl,
//     on the metric tables those kernels read: the spacings of an "exactly uniform" grid may scatter by a few ulp, ins_grid.hip), workgroup partials go
//     to a [member][chunk] array of the handle, and a second kernel, one workgroup per member, combines them in a fixed order. No floating-point atomics: results are deterministic and do not depend on B.  max and min are
//     exact, so those two values are bitwise the per-member entries'; the energy is the same non-negative terms summed in another order.
//   * ins_rk_ensemble_spectrum_f64: the x pass of the solver (k_xfwd with MEMBERS, ins_fft.hip) fed from the velocity components with their ghosts stripped in the
//     load, the forward y pass k_yfft over the [ky][2·member + component][kxs] layout it leaves (the lines of all members side by side in every ky row: one
//     plane of 2·B·kxs columns), and the chunked shell sums of ins_spectrum.hip with a member dimension.  Four launches, no FFT-library call.  The index sets
//     are re-addressed once, at creation, to the storage order the y pass leaves ky in.
#include "ins_debug.h"
#include "ins_internal.h"

struct ins_ensemble_spectrum {
  ins_rk_ensemble* ens = nullptr;  // borrowed
  int nbin = 0, nb = 0, n0 = 0, n1 = 0, kxs = 0;
  double scale = 0.0;
  DevBuf<double> tw[2];
  DevBuf<double> hat;            // n1 · 2 nb · kxs complex
  DevBuf<long long> inds;        // positions inside one line set of `hat`: kx + (2 nb kxs) · (storage position of ky)
  int nchunk = 0;
  DevBuf<long long> chunk_lo, chunk_hi;
  DevBuf<int> bin_chunk0;        // nbin + 1: first chunk of every shell
  DevBuf<double> partial;        // [member][component][chunk]
};

namespace {

constexpr int ST_ROWS = 16;  // rows per workgroup of the statistics kernel: four per wavefront

struct StatsMetric {
  double dt_diff[2];  // Re min(Δu)² / 2 per direction
};

// in-order tree over the 64 lanes: the same shape whatever the data
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}

// blockIdx.z = member, blockIdx.x = tile of 64 columns, blockIdx.y = chunk of ST_ROWS rows; wavefront threadIdx.y marches its ST_ROWS / 4 rows upwards and
// carries the y-component of the row below in a register; the x neighbour is a reload of the line the wavefront has just read.  Ghost volumes of U are valid
// (the contract of ins_rk_ensemble_rhs_f64): every interior volume is a DOF of both components, so one walk over Ip serves all three quantities.
__global__ __launch_bounds__(256) void k_ensemble_stats(GridDev g, const double* __restrict__ U, long long ustride, int n0, int n1, double* __restrict__ part) {
  __shared__ double red[3][4];
  const double* u0 = U + (long long)blockIdx.z * ustride;
  const double* u1 = u0 + g.sc;
  const int N0 = g.N[0];
  const int i = blockIdx.x * 64 + threadIdx.x;
  const int w = threadIdx.y;
  const int jb = blockIdx.y * ST_ROWS + w * (ST_ROWS / 4);
  const bool col = i < n0;
  const int ic = col ? i : n0 - 1;  // stay in memory; the lane's values are not counted
  double e_acc = 0.0, d_acc = 0.0, c_acc = INFINITY;
  if (jb < n1) {
    const int I0 = g.ip_lo[0] + ic;
    const double dx0 = g.dx[0][I0], rdx0 = g.rdx[0][I0], dxu0 = g.dxu[0][I0];
    long long c = (long long)I0 + (long long)(g.ip_lo[1] + jb) * N0;
    double vm = u1[c - N0];
    const int je = min(jb + ST_ROWS / 4, n1);
    for (int j = jb; j < je; ++j, c += N0) {
      const int I1 = g.ip_lo[1] + j;
      const double om = dx0 * g.dx[1][I1], rdx1 = g.rdx[1][I1], dxu1 = g.dxu[1][I1];
      const double up0 = u0[c], um0 = u0[c - 1], up1 = u1[c], um1 = vm;
      vm = up1;
      // kinetic_energy! (interpolate_first = false) · Ω                                   k_kinetic_energy, k_scalewithvolume
      double e = 0.0;
      e += up0 * up0 + um0 * um0;
      e += up1 * up1 + um1 * um1;
      double ke = e / 4;
      ke *= om;
      // divergence!                                                                      k_divergence
      double d = 0.0;
      d += (up0 - um0) * rdx0;
      d += (up1 - um1) * rdx1;
      // Δu[α] / |u[α]|                                                                    k_cfl
      const double c0 = dxu0 / fabs(up0), c1 = dxu1 / fabs(up1);
      if (col) {
        e_acc += ke;
        d_acc = fmax(d_acc, fabs(d));
        c_acc = fmin(c_acc, fmin(c0, c1));
      }
    }
  }
  e_acc = wave_sum(e_acc);
  d_acc = wave_max(d_acc);
  c_acc = wave_min(c_acc);
  if (threadIdx.x == 0) {
    red[0][w] = e_acc;
    red[1][w] = d_acc;
    red[2][w] = c_acc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && w == 0) {
    const long long chunk = (long long)blockIdx.y * gridDim.x + blockIdx.x, nchunk = (long long)gridDim.x * gridDim.y;
    double* p = part + ((long long)blockIdx.z * nchunk + chunk) * 3;
    p[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    p[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    p[2] = fmin(fmin(red[2][0], red[2][1]), fmin(red[2][2], red[2][3]));
  }
}

// one workgroup (one wavefront) per member: lane l takes chunks l, l + 64, .. in order, then the lane tree
__global__ __launch_bounds__(64) void k_ensemble_stats_finish(const double* __restrict__ part, int nchunk, StatsMetric m, double* __restrict__ out) {
  const double* p = part + (long long)blockIdx.x * nchunk * 3;
  double e = 0.0, d = 0.0, c = INFINITY;
  for (int q = threadIdx.x; q < nchunk; q += 64) {
    e += p[3 * q];
    d = fmax(d, p[3 * q + 1]);
    c = fmin(c, p[3 * q + 2]);
  }
  e = wave_sum(e);
  d = wave_max(d);
  c = wave_min(c);
  if (threadIdx.x == 0) {
    double* o = out + 3LL * blockIdx.x;
    o[0] = e;
    o[1] = d;
    o[2] = fmin(fmin(m.dt_diff[0], m.dt_diff[1]), c);  // get_cfl_timestep!: min over directions of min(Δt_diff, Δt_conv)      solver.jl:108-121
  }
}

// k_shell_chunks of ins_spectrum.hip with a member dimension: blockIdx.x = chunk of the index list (inside one shell), blockIdx.y = 2·member + component
__global__ __launch_bounds__(256) void k_shell_chunks_members(const double2* __restrict__ hat, int kxs, const long long* __restrict__ lo,
                                                              const long long* __restrict__ hi, const long long* __restrict__ inds,
                                                              double* __restrict__ partial) {
  __shared__ double red[4];
  const double2* line = hat + (long long)blockIdx.y * kxs;
  double acc = 0.0;
  for (long long q = lo[blockIdx.x] + threadIdx.x; q < hi[blockIdx.x]; q += 256) {
    const double2 v = line[inds[q]];
    acc += v.x * v.x + v.y * v.y;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// one work-item per (shell, member): per component its chunk sums in order, the components added as ins_spectrum_f64 adds them
__global__ __launch_bounds__(64) void k_shell_finish_members(const int* __restrict__ bin_chunk0, const double* __restrict__ partial, int nchunk, int nbin,
                                                             double scale, double* __restrict__ ehat) {
  const int bin = blockIdx.x * 64 + threadIdx.x;
  if (bin >= nbin) return;
  double e = 0.0;
  for (int a = 0; a < 2; ++a) {
    const double* p = partial + ((long long)blockIdx.y * 2 + a) * nchunk;
    double acc = 0.0;
    for (int c = bin_chunk0[bin]; c < bin_chunk0[bin + 1]; ++c) acc += p[c];
    e += scale * acc;
  }
  ehat[(long long)blockIdx.y * nbin + bin] = e;
}

}  // namespace

extern "C" int ins_rk_ensemble_stats_f64(ins_rk_ensemble_t* e, double Re, const double* U, int64_t ustride, double* out, void* stream) {
  INS_REQUIRE(e && U && out, "null argument");
  int rc = ins_rk_ensemble_check_observer(e, "ins_rk_ensemble_stats_f64", ustride);
  if (rc) return rc;
  const ins_grid* G = e->grid;
  const GridDev& g = G->g;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      INS_REQUIRE(g.iu_lo[a][b] == g.ip_lo[b] && g.iu_hi[a][b] == g.ip_hi[b] && g.ip_lo[b] >= 1, "ensemble statistics: every interior volume must be a velocity DOF");
  const int n0 = g.ip_hi[0] - g.ip_lo[0], n1 = g.ip_hi[1] - g.ip_lo[1];
  StatsMetric m;
  for (int a = 0; a < 2; ++a) {
    double damin = INFINITY;
    for (int i = g.iu_lo[a][a]; i < g.iu_hi[a][a]; ++i) damin = fmin(damin, G->desc.dxu[a][i]);
    m.dt_diff[a] = Re * damin * damin / 2;
  }
  const dim3 grid(cdiv(n0, 64), cdiv(n1, ST_ROWS), (unsigned)e->nb);
  const size_t nchunk = (size_t)grid.x * grid.y;
  if ((rc = e->stats_part.ensure(nchunk * 3 * e->nb))) return rc;  // first call only
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(k_ensemble_stats, grid, dim3(64, 4, 1), 0, s, g, U, (long long)ustride, n0, n1, e->stats_part.get());
  INS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ensemble_stats_finish, dim3((unsigned)e->nb), dim3(64), 0, s, (const double*)e->stats_part.get(), (int)nchunk, m, out);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

extern "C" int ins_rk_ensemble_spectrum_destroy(ins_ensemble_spectrum_t* S) {
  if (!S) return INS_OK;
  delete S;
  return INS_OK;
}

extern "C" int ins_rk_ensemble_spectrum_create(ins_rk_ensemble_t* e, int nbin, const int64_t* offsets, const int64_t* inds, ins_ensemble_spectrum_t** out) {
  INS_REQUIRE(e && offsets && inds && out && nbin >= 1, "bad argument");
  int rc = ins_rk_ensemble_check_observer(e, "ins_rk_ensemble_spectrum_create", 2 * e->grid->ncell);
  if (rc) return rc;
  INS_REQUIRE(e->nb <= 32767, "member spectrum: at most 32767 members (two lines per member in one launch dimension)");
  const GridDev& g = e->grid->g;
  ins_ensemble_spectrum* S = new ins_ensemble_spectrum();
  S->ens = e;
  S->nbin = nbin;
  S->nb = e->nb;
  S->n0 = g.ip_hi[0] - g.ip_lo[0];
  S->n1 = g.ip_hi[1] - g.ip_lo[1];
  const long long ntot = (long long)S->n0 * S->n1;
  S->scale = 1.0 / (2.0 * (double)ntot * (double)ntot);
  S->kxs = (S->n0 / 2 + 1 + 7) & ~7;  // rows padded to whole 128-B lines, as in the Poisson solver
  const long long rs = (long long)S->kxs * 2 * S->nb;  // one ky row down
  const int K0 = S->n0 / 2, K1 = S->n1 / 2;
  // storage position of ky after the forward y pass: ins_ownfft_permute_symbol writes out[pos(k)] = in[k]
  std::vector<double> ident((size_t)S->n1), freq_at((size_t)S->n1);
  for (int k = 0; k < S->n1; ++k) ident[k] = k;
  ins_ownfft_permute_symbol(S->n1, ident.data(), freq_at.data());
  std::vector<int> pos_of((size_t)S->n1);
  for (int p = 0; p < S->n1; ++p) pos_of[(int)freq_at[p]] = p;
  // index sets address the K-array of the reference (column-major over K0 x K1): re-address them inside one line set of `hat`
  const long long nind = offsets[nbin], nk = (long long)K0 * K1;
  std::vector<long long> pos((size_t)nind);
  for (long long q = 0; q < nind; ++q) {
    const long long mm = inds[q];
    if (mm < 0 || mm >= nk) {
      delete S;
      ins_set_error("spectrum index %lld outside the %lld retained modes", mm, nk);
      return INS_ERR_INVALID;
    }
    pos[q] = mm % K0 + rs * pos_of[mm / K0];
  }
  // chunks of the index list, none crossing a shell (as ins_spectrum_create)
  constexpr long long CH = 4096;
  std::vector<long long> clo, chi;
  std::vector<int> bc0(nbin + 1, 0);
  for (int b = 0; b < nbin; ++b) {
    bc0[b] = (int)clo.size();
    for (long long q = offsets[b]; q < offsets[b + 1]; q += CH) {
      clo.push_back(q);
      chi.push_back(std::min<long long>(q + CH, offsets[b + 1]));
    }
  }
  bc0[nbin] = (int)clo.size();
  S->nchunk = (int)clo.size();
  const size_t nc = std::max<size_t>(clo.size(), 1);
  // padding columns of `hat` are written by no pass: zeroed once, they stay zero through the y pass
  (rc = S->hat.alloc_zero((size_t)rs * S->n1 * 2)) || (rc = ins_zsolve_twiddles(S->n0, &S->tw[0])) || (rc = ins_zsolve_twiddles(S->n1, &S->tw[1])) ||
      (rc = S->inds.alloc(std::max<long long>(nind, 1))) || (rc = nind ? ins_devmem_copy_from_host(S->inds, pos.data(), nind * sizeof(long long)) : INS_OK) ||
      (rc = S->chunk_lo.alloc(nc)) || (rc = S->chunk_hi.alloc(nc)) || (rc = S->bin_chunk0.alloc_copy_host(nbin + 1, bc0.data())) ||
      (rc = S->partial.alloc_zero(nc * 2 * S->nb));
  if (rc == INS_OK && !clo.empty())
    (rc = ins_devmem_copy_from_host(S->chunk_lo, clo.data(), clo.size() * sizeof(long long))) ||
        (rc = ins_devmem_copy_from_host(S->chunk_hi, chi.data(), chi.size() * sizeof(long long)));
  if (rc != INS_OK) {
    delete S;
    return rc;
  }
  *out = S;
  return INS_OK;
}

extern "C" int ins_rk_ensemble_spectrum_f64(ins_ensemble_spectrum_t* S, const double* U, int64_t ustride, double* ehat, void* stream) {
  INS_REQUIRE(S && U && ehat, "null argument");
  int rc = ins_rk_ensemble_check_observer(S->ens, "ins_rk_ensemble_spectrum_f64", ustride);
  if (rc) return rc;
  INS_REQUIRE(S->ens->nb == S->nb, "the ensemble handle has changed since the spectrum was created");
  hipStream_t s = as_stream(stream);
  const int lines = 2 * S->nb * S->kxs;  // columns of one ky row
  if ((rc = ins_k_ownfft_xfwd_field_members(S->ens->grid, U, ustride, S->hat, S->n0, S->n1, S->nb, S->tw[0], s, S->kxs))) return rc;
  if ((rc = ins_k_ownfft_y(S->hat, lines, S->n1, 1, S->tw[1], false, s, lines))) return rc;
  if (S->nchunk) {
    hipLaunchKernelGGL(k_shell_chunks_members, dim3((unsigned)S->nchunk, 2u * S->nb), dim3(256), 0, s, reinterpret_cast<const double2*>(S->hat.get()), S->kxs,
                       S->chunk_lo.get(), S->chunk_hi.get(), S->inds.get(), S->partial.get());
    INS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_shell_finish_members, dim3(cdiv(S->nbin, 64), (unsigned)S->nb), dim3(64), 0, s, S->bin_chunk0.get(), (const double*)S->partial.get(),
                     std::max(S->nchunk, 1), S->nbin, S->scale, ehat);
  INS_LAUNCH_CHECK();
  return INS_OK;
}
