// The `_f32` entry-point family ("leaves `_f32` as a suffix-parallel family"; the reference is generic in the element
// type and recommends single precision on GPUs, docs/src/manual/precision.md:3-16; examples/DecayingTurbulence3D.jl:16 runs T = Float32).
//
// Scope: all-periodic uniform boxes, 2-D and 3-D — the configuration the reference's own Float32 example runs (spectral pressure solver).
//   K1 (momentum!)          : the 64-outputs-per-wavefront stage kernel of ins_flux64.hip instantiated for float (wide 3-D boxes: half
//                             the bytes of the fp64 kernel at the same memory rate), a plain one-cell-per-work-item kernel elsewhere;
//   spectral projection     : 3-D power-of-two boxes: the library's five fused fp64 passes, the right-hand side Ω·div(u) formed from the float field
//                             inside the x pass (ins_fft.hip, SRC = 5) — a mixed-precision projection whose pressure is more accurate than a
//                             float solve; other boxes: Ω·div(u) -> hipFFT R2C -> symbol -> C2R; then padded p with periodic ghosts,
//                             u -= ∇p, periodic ghosts of u;
//   explicit RK             : the stage loop of step_explicit_runge_kutta.jl:4-59 on those kernels, the stage combination as K1's epilogue
//                             on wide 3-D boxes.
// Arrays are the reference layout with Float32 elements.  The grid handle is the fp64 one (metrics are computed in double and rounded
// once per launch).  Non-periodic or stretched grids return INS_ERR_UNSUPPORTED: no silent fp64 fallback.
#include <cmath>
#include <cstdlib>

#include "ins_debug.h"
#include "ins_f32_internal.h"
#include "ins_rk_terms.h"

struct ins_poisson32 {
  const ins_grid* grid = nullptr;  // borrowed
  // which launch sequence this solver runs: what its creation actually set up (ins_f32_choose; ins_poisson_wrap_f32).  The pointers below are resources
  // of a route, never tests of it.
  F32Route route = F32_HIPFFT;
  hipfftHandle fwd = 0, inv = 0;
  bool plans = false;
  DevBuf<float> pI;
  DevBuf<hipfftComplex> phat;
  DevBuf<float> ahat[3];
  int np[3] = {1, 1, 1}, kmax[3] = {1, 1, 1};
  // 3-D power-of-two boxes: project! solves its pressure equation with the library's fused fp64 passes (right-hand side formed from the
  // float field inside the x pass, five passes instead of hipFFT's 3-D plans + separate kernels; the pressure is MORE accurate than a float
  // solve would give).  512^3 RK44 step: 26.9 ms with hipFFT's float plans -> see DESIGN.md §5.
  ins_poisson* ps64 = nullptr;  // owned: ins_poisson_destroy
  // sides the three-pass z kernel takes (192, 256, 384, 512 planes): the same five passes on FLOAT2 spectra — half the bytes of every pass; ps64
  // then only supplies the symbol vectors (INS_F32_FP64_SPECTRA=1 keeps the fp64 passes)
  DevBuf<float> phat32;
  DevBuf<float> tw32[3];
  int kxs32 = 0;
  // ins_poisson_wrap_f32: a Float32 solver around a caller-owned fp64 solver of any kind (walls / stretched grids: psolver_direct, psolver_cg)
  ins_poisson* wrap64 = nullptr;  // borrowed
  DevBuf<double> p64;   // padded fp64 right-hand side / solution
  DevBuf<float> div32;  // padded scratch of the divergence diagnostic
};

struct ins_rk32 {
  const ins_grid* grid = nullptr;  // borrowed
  ins_poisson32* ps = nullptr;     // borrowed
  int nstage = 0;
  std::vector<double> A, c;
  std::vector<DevBuf<float>> ku;
  DevBuf<float> ub[2];
  DevBuf<float> p;
  DevBuf<float> pu;  // unpadded float copy of the stage pressure (in-register correction of the next stage's stencil kernel)
  DevBuf<float> ustart;  // chained steps: the corrected start field of steps 2..K (the caller's array holds the uncorrected last stage velocity then)
  // temperature equation (ins_rk_set_temperature_f32, ins_rk_step_ext_f32): scalar scratch allocated by the first step that carries a temperature
  bool temp_on = false;
  ins_temperature_desc_t td = {};
  DevBuf<float> tempstart;
  DevBuf<float> tstage;         // the one stage temperature buffer: stage temperatures alternate between it and the caller's array
  DevBuf<float> diff;           // scratch of dissipation! (vector field)
  std::vector<DevBuf<float>> ktemp;  // nstage scalars
  // Smagorinsky closure and steady body force (ins_rk_set_closure_f32, ins_rk_set_bodyforce_f32)
  int closure = 0;              // 0 none, 1 Smagorinsky
  float theta = 0.f;
  const float* force = nullptr; // borrowed: the caller's device field
  DevBuf<float> E;              // closure force (vector field; only its degrees of freedom are ever written)
  DevBuf<float> sigma;          // D(D+1)/2 scalar fields (three-kernel route)
};

namespace {

struct Box32 {
  int D, N[3], n[3];
  long long sx[3], sc;
  float rh[3];  // 1/h
  float om;     // cell volume
};

Box32 box_of(const ins_grid* G) {
  Box32 b;
  const GridDev& g = G->g;
  b.D = g.D;
  double om = 1.0;
  for (int a = 0; a < 3; ++a) {
    b.N[a] = a < g.D ? g.N[a] : 1;
    b.n[a] = a < g.D ? g.N[a] - 2 : 1;
    b.sx[a] = g.sx[a];
    b.rh[a] = a < g.D ? (float)(1.0 / G->h[a]) : 0.f;
    if (a < g.D) om *= G->h[a];
  }
  b.sc = g.sc;
  b.om = (float)om;
  return b;
}

int require_periodic_uniform(const ins_grid* G, const char* what) {
  if (!(G->all_periodic && G->uniform)) {
    ins_set_error("%s: all-periodic uniform boxes only (other grids: ins_poisson_wrap_f32 around psolver_direct / psolver_cg)", what);
    return INS_ERR_UNSUPPORTED;
  }
  return INS_OK;
}
inline bool periodic_uniform(const ins_grid* G) { return G->all_periodic && G->uniform; }

// ghost volumes of `ncomp` components: cell 0 <- cell N-2, cell N-1 <- cell 1, direction after direction (corners consistent),
// boundary_conditions.jl:276-288 / 306-318
__global__ __launch_bounds__(256) void k32_bc_periodic(Box32 b, float* __restrict__ f, int ncomp, int dir) {
  const int d1 = (dir + 1) % 3, d2 = (dir + 2) % 3;
  const long long plane = (long long)b.N[d1] * b.N[d2];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < plane * ncomp; t += (long long)gridDim.x * 256) {
    const int c = (int)(t / plane);
    const long long r = t % plane;
    const int i1 = (int)(r % b.N[d1]), i2 = (int)(r / b.N[d1]);
    float* base = f + c * b.sc + i1 * b.sx[d1] + i2 * b.sx[d2];
    base[0] = base[(long long)(b.N[dir] - 2) * b.sx[dir]];
    base[(long long)(b.N[dir] - 1) * b.sx[dir]] = base[b.sx[dir]];
  }
}

int bc_periodic(const ins_grid* G, float* f, int ncomp, hipStream_t s) {
  const Box32 b = box_of(G);
  for (int dir = 0; dir < b.D; ++dir) {
    const long long work = (long long)b.N[(dir + 1) % 3] * b.N[(dir + 2) % 3] * ncomp;
    hipLaunchKernelGGL(k32_bc_periodic, dim3((unsigned)std::min<long long>((work + 255) / 256, 4096)), dim3(256), 0, s, b, f, ncomp, dir);
  }
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// momentum! on a uniform periodic box, one cell per work-item (operators.jl:647-690 with every weight 1/2 and constant spacings);
// u needs valid ghosts.  FUSE-free: the wide 3-D boxes take ins_flux64.hip's kernel instead.
template <int D>
__global__ __launch_bounds__(256) void k32_momentum(Box32 b, float visc, const float* __restrict__ u, float* __restrict__ F) {
  const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y, k = D == 3 ? 1 + (int)blockIdx.z : 0;
  if (i > b.n[0] || j > b.n[1]) return;
  const long long c = i + j * b.sx[1] + k * b.sx[2];
#pragma unroll
  for (int al = 0; al < D; ++al) {
    const float* ua = u + al * b.sc;
    float f = 0.f;
#pragma unroll
    for (int be = 0; be < D; ++be) {
      const float* ub = u + be * b.sc;
      const long long sb = b.sx[be], sa = b.sx[al];
      const float uc = ua[c], um = ua[c - sb], up = ua[c + sb];
      const float uab1 = 0.5f * (um + uc), uab2 = 0.5f * (uc + up);
      const float uba1 = 0.5f * (ub[c - sb] + ub[c - sb + sa]), uba2 = 0.5f * (ub[c] + ub[c + sa]);
      const float d1 = (uc - um) * b.rh[be], d2 = (up - uc) * b.rh[be];
      f += (visc * (d2 - d1) - (uab2 * uba2 - uab1 * uba1)) * b.rh[be];
    }
    F[al * b.sc + c] = f;
  }
}

// pI = Ω div(u) with the periodic image of u[I - e_a] (no ghost fill of u needed)        operators.jl:117-125, 81-95, pressure.jl:320
template <int D>
__global__ __launch_bounds__(256) void k32_div(Box32 b, const float* __restrict__ u, float* __restrict__ pI) {
  const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y * 4 + threadIdx.y, kk = D == 3 ? (int)blockIdx.z : 0;
  if (ii >= b.n[0] || jj >= b.n[1]) return;
  const int I[3] = {ii + 1, jj + 1, D == 3 ? kk + 1 : 0};
  const long long c = I[0] + I[1] * b.sx[1] + I[2] * b.sx[2];
  float d = 0.f;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float* ua = u + a * b.sc;
    const long long cm = I[a] == 1 ? c + (long long)(b.N[a] - 3) * b.sx[a] : c - b.sx[a];
    d += (ua[c] - ua[cm]) * b.rh[a];
  }
  pI[ii + (long long)b.n[0] * (jj + (long long)b.n[1] * kk)] = d * b.om;
}

// phat = -phat / (ax + ay + az) / prod(Np), phat[0] = 0                                  pressure.jl:326-341
template <int D>
__global__ __launch_bounds__(256) void k32_symbol(hipfftComplex* __restrict__ phat, const float* __restrict__ ax, const float* __restrict__ ay,
                                                  const float* __restrict__ az, int k0, int k1, float inv_n) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = D == 3 ? (int)blockIdx.z : 0;
  if (i >= k0 || j >= k1) return;
  const long long q = i + (long long)k0 * (j + (long long)k1 * k);
  float den = ax[i] + ay[j];
  if (D == 3) den += az[k];
  const float sc = (i == 0 && j == 0 && k == 0) ? 0.f : -inv_n / den;
  hipfftComplex v = phat[q];
  v.x *= sc;
  v.y *= sc;
  phat[q] = v;
}

// p (padded, with periodic ghosts) <- pI; one work-item per padded volume                pressure.jl:347, boundary_conditions.jl:306-318
template <int D, typename S = float>
__global__ __launch_bounds__(256) void k32_pad(Box32 b, const S* __restrict__ pI, float* __restrict__ p) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, k = D == 3 ? (int)blockIdx.z : 0;
  if (i >= b.N[0] || j >= b.N[1]) return;
  auto w = [](int I, int n) { return I == 0 ? n - 1 : (I == n + 1 ? 0 : I - 1); };
  const long long q = w(i, b.n[0]) + (long long)b.n[0] * (w(j, b.n[1]) + (long long)b.n[1] * (D == 3 ? w(k, b.n[2]) : 0));
  p[i + j * b.sx[1] + k * b.sx[2]] = (float)pI[q];
}

// u[I, a] -= (p[I + e_a] - p[I]) / h_a on the interior                                    operators.jl:225-233
template <int D>
__global__ __launch_bounds__(256) void k32_applypressure(Box32 b, float* __restrict__ u, const float* __restrict__ p) {
  const int i = 1 + blockIdx.x * 64 + threadIdx.x, j = 1 + blockIdx.y * 4 + threadIdx.y, k = D == 3 ? 1 + (int)blockIdx.z : 0;
  if (i > b.n[0] || j > b.n[1]) return;
  const long long c = i + j * b.sx[1] + k * b.sx[2];
  const float pc = p[c];
#pragma unroll
  for (int a = 0; a < D; ++a) u[a * b.sc + c] -= (p[c + b.sx[a]] - pc) * b.rh[a];
}

// The three kernels above as one pass (3-D): every interior volume reads its own velocity and p at itself and its three upper periodic
// images from the unpadded solver output, and writes u - ∇p and p to itself and to the ghost volumes it is the image of (the fp64 path's
// k_grad_ghost3, ins_poisson.hip).  512^3: pad 0.39 + gradient 0.82 + six ghost-strip kernels -> one pass.
template <typename S>
__global__ __launch_bounds__(256) void k32_grad_ghost3(Box32 b, float* __restrict__ u, float* __restrict__ p, const S* __restrict__ pI) {
  const int ii = blockIdx.x * 64 + threadIdx.x, jj = blockIdx.y * 4 + threadIdx.y, kk = blockIdx.z;
  if (ii >= b.n[0] || jj >= b.n[1]) return;
  const int w[3] = {ii, jj, kk};
  const int I[3] = {ii + 1, jj + 1, kk + 1};
  const long long qs[3] = {1, b.n[0], (long long)b.n[0] * b.n[1]};
  const long long q = ii + qs[1] * jj + qs[2] * kk;
  const long long c = I[0] + I[1] * b.sx[1] + I[2] * b.sx[2];
  const float pc = (float)pI[q];
  float un[3];
  int img[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const long long qn = (w[a] + 1 < b.n[a]) ? q + qs[a] : q - (long long)(b.n[a] - 1) * qs[a];
    un[a] = u[a * b.sc + c] - ((float)pI[qn] - pc) * b.rh[a];
    img[a] = I[a] == 1 ? b.N[a] - 1 : (I[a] == b.N[a] - 2 ? 0 : -1);
  }
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    bool ok = true;
    long long cc = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const bool use = (m >> a) & 1;
      ok = ok && (!use || img[a] >= 0);
      cc += (long long)(use ? img[a] : I[a]) * b.sx[a];
    }
    if (ok) {
      u[cc] = un[0];
      u[cc + b.sc] = un[1];
      u[cc + 2 * b.sc] = un[2];
      p[cc] = pc;
    }
  }
}

// out = base + Σ coef_q k_q                                                             step_explicit_runge_kutta.jl:35-38
struct Comb32 {
  int n;
  float coef[INS_MAX_STAGES + 1];
  const float* k[INS_MAX_STAGES + 1];
};
__global__ __launch_bounds__(256) void k32_combine(long long n, const float* __restrict__ base, float* __restrict__ out, Comb32 cb) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    float v = base[t];
    for (int q = 0; q < cb.n; ++q) v += cb.coef[q] * cb.k[q][t];
    out[t] = v;
  }
}

// a += b (the closure force joins the stage force)                                     step_explicit_runge_kutta.jl:31-34
__global__ __launch_bounds__(256) void k32_add(long long n, float* __restrict__ a, const float* __restrict__ b) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) a[t] += b[t];
}

__global__ __launch_bounds__(256) void k32_cvt(long long n, const double* __restrict__ a, float* __restrict__ b) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) b[t] = (float)a[t];
}

dim3 grid_over(const Box32& b, bool padded) {
  const int e0 = padded ? b.N[0] : b.n[0], e1 = padded ? b.N[1] : b.n[1], e2 = b.D == 3 ? (padded ? b.N[2] : b.n[2]) : 1;
  return dim3(cdiv(e0, 64), cdiv(e1, 4), e2);
}

// kern<2> on a 2-D box, kern<3> on a 3-D one, 64 x 4 work-items a block
#define K32_LAUNCH_BY_DIM(D, kern, grid, s, ...)                                         \
  do {                                                                                   \
    if ((D) == 2) hipLaunchKernelGGL(kern<2>, grid, dim3(64, 4), 0, s, __VA_ARGS__);     \
    else hipLaunchKernelGGL(kern<3>, grid, dim3(64, 4), 0, s, __VA_ARGS__);              \
  } while (0)

void pad32(const Box32& b, const float* pI, float* p, hipStream_t s) { K32_LAUNCH_BY_DIM(b.D, k32_pad, grid_over(b, true), s, b, pI, p); }
void pad32(const Box32& b, const double* pI, float* p, hipStream_t s) {  // the fp64 passes exist in 3-D only
  hipLaunchKernelGGL((k32_pad<3, double>), grid_over(b, true), dim3(64, 4), 0, s, b, pI, p);
}

// The tail of project!: pI (unpadded, float or double) -> p with ghosts, u -= ∇p with ghosts, as one kernel (3-D) or pad -> gradient-subtract -> periodic ghosts
template <typename S>
int project_tail(const ins_grid* G, const Box32& b, float* u, float* p, const S* pI, bool one_kernel, hipStream_t s) {
  if (one_kernel) {
    hipLaunchKernelGGL((k32_grad_ghost3<S>), grid_over(b, false), dim3(64, 4), 0, s, b, u, p, pI);
    INS_LAUNCH_CHECK();
    return INS_OK;
  }
  pad32(b, pI, p, s);
  K32_LAUNCH_BY_DIM(b.D, k32_applypressure, grid_over(b, false), s, b, u, p);
  INS_LAUNCH_CHECK();
  return bc_periodic(G, u, b.D, s);
}

// maximum(abs, dev[0..n)) on the host (blocking)
int host_max_abs(const float* dev, long long n, hipStream_t s, float* out) {
  std::vector<float> h(n);
  INS_HIP_TRY(hipMemcpyAsync(h.data(), dev, n * sizeof(float), hipMemcpyDeviceToHost, s));
  INS_HIP_TRY(hipStreamSynchronize(s));
  *out = 0.f;
  for (float v : h) *out = std::fmax(*out, std::fabs(v));
  return INS_OK;
}

}  // namespace

// out = base + Σ coef[q] k[q], terms in index order; serves this file's stage loops and the recomputation of the reverse loop (ins_rk_adjoint_loop.h)
int ins_k32_combine(long long n, const float* base, float* out, int nterms, const float* coef, const float* const* k, hipStream_t s) {
  Comb32 cb;
  cb.n = nterms;
  for (int q = 0; q < nterms; ++q) {
    cb.coef[q] = coef[q];
    cb.k[q] = k[q];
  }
  hipLaunchKernelGGL(k32_combine, dim3((unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 8192))), dim3(256), 0, s, n, base, out, cb);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

extern "C" int ins_apply_bc_u_f32(const ins_grid_t* G, float* u, void* stream) {
  INS_REQUIRE(G && u, "null argument");
  if (!periodic_uniform(G)) return ins_k32g_apply_bc_u(G, u, as_stream(stream));
  return bc_periodic(G, u, G->g.D, as_stream(stream));
}

// apply_bc_u!(u, t, setup; dudt = true): the ghost fill of a time derivative — constant Dirichlet data contributes zero.  Periodic copies are the same.
extern "C" int ins_apply_bc_u_dudt_f32(const ins_grid_t* G, float* u, void* stream) {
  INS_REQUIRE(G && u, "null argument");
  if (!periodic_uniform(G)) return ins_k32g_apply_bc_u(G, u, as_stream(stream), 1);
  return bc_periodic(G, u, G->g.D, as_stream(stream));
}

extern "C" int ins_apply_bc_p_f32(const ins_grid_t* G, float* p, void* stream) {
  INS_REQUIRE(G && p, "null argument");
  if (!periodic_uniform(G)) return ins_k32g_apply_bc_p(G, p, as_stream(stream));
  return bc_periodic(G, p, 1, as_stream(stream));
}

extern "C" int ins_momentum_f32(const ins_grid_t* G, float visc, const float* u, float* F, void* stream) {
  INS_REQUIRE(G && u && F, "null argument");
  hipStream_t s = as_stream(stream);
  if (!periodic_uniform(G)) return ins_k32g_momentum(G, visc, u, F, s);
  if (ins_flux64_supported(G)) return ins_k_flux64_f32(G, (double)visc, u, F, nullptr, nullptr, 0, s);
  const Box32 b = box_of(G);
  K32_LAUNCH_BY_DIM(b.D, k32_momentum, grid_over(b, false), s, b, visc, u, F);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

extern "C" int ins_poisson_destroy_f32(ins_poisson32_t* ps) {
  if (!ps) return INS_OK;
  if (ps->plans) {
    (void)hipfftDestroy(ps->fwd);
    (void)hipfftDestroy(ps->inv);
  }
  if (ps->ps64) (void)ins_poisson_destroy(ps->ps64);
  delete ps;  // wrap64 is the caller's
  return INS_OK;
}

// A Float32 pressure solver around ANY fp64 solver of the same grid (psolver_direct, psolver_cg, psolver_spectral; pressure.jl:85-154, 209-351): the
// right-hand side is formed / widened in double, the fp64 solver runs unchanged, the pressure is rounded to float once.  `ps64` stays the caller's and must
// outlive the returned handle.  This is what carries the `_f32` family to wall-bounded and stretched grids (csrc/ins_f32g.hip).
extern "C" int ins_poisson_wrap_f32(const ins_grid_t* G, ins_poisson_t* ps64, ins_poisson32_t** out) {
  INS_REQUIRE(G && ps64 && out, "null argument");
  INS_REQUIRE(ps64->grid == G, "the fp64 solver was created for a different grid");
  const GridDev& g = G->g;
  for (int a = 0; a < g.D; ++a)
    if (g.bc[a][0] == INS_BC_HALO || g.bc[a][1] == INS_BC_HALO) {
      ins_set_error("ins_poisson_wrap_f32: slab (halo) grids run in fp64 only");
      return INS_ERR_UNSUPPORTED;
    }
  ins_poisson32* ps = new ins_poisson32();
  ps->grid = G;
  ps->route = F32_WRAP;
  ps->wrap64 = ps64;
  for (int a = 0; a < g.D; ++a) ps->np[a] = g.ip_hi[a] - g.ip_lo[a];
  int rc;
  if ((rc = ps->p64.alloc_zero(G->ncell)) || (rc = ps->div32.alloc_zero(G->ncell))) {
    ins_poisson_destroy_f32(ps);
    return rc;
  }
  *out = ps;
  return INS_OK;
}

// Which launch sequence an all-periodic uniform box of n0 x n1 (x n2) volumes gets: a function of the box and of the option values at the time of the call, with
// no HIP call.  ins_poisson_spectral_create_f32 calls it once, so INS_F32_HIPFFT_PROJECT, INS_F32_FP64_SPECTRA and the switches behind the two predicates
// (ins_spectral_choose's, INS_DISABLE_ZSOLVE) are frozen in a solver that exists; INS_F32_SPLIT_GRADIENT alone is read per call (ins_project_f32).
F32Route ins_f32_choose(int D, int n0, int n1, int n2) {
  if (D != 3 || ins_opt(OPT_INS_F32_HIPFFT_PROJECT)) return F32_HIPFFT;
  if (ins_dbg_spectral_choose(D, n0, n1, n2, nullptr, nullptr) < ROUTE_OWN2D) return F32_HIPFFT;  // the fp64 solver of this box has no own passes
  return ins_zsolve_f32_supported(n2) && !ins_opt(OPT_INS_F32_FP64_SPECTRA) ? F32_FLOAT2_SPECTRA : F32_FP64_SPECTRA;
}

// psolver_spectral(setup) with T = Float32                                               pressure.jl:289-351
extern "C" int ins_poisson_spectral_create_f32(const ins_grid_t* G, ins_poisson32_t** out) {
  INS_REQUIRE(G && out, "null argument");
  int rc = require_periodic_uniform(G, "ins_poisson_spectral_create_f32");
  if (rc) return rc;
  const GridDev& g = G->g;
  ins_poisson32* ps = new ins_poisson32();
  ps->grid = G;
  long long nreal = 1, ncplx = 1;
  double om = 1.0;
  for (int a = 0; a < g.D; ++a) {
    ps->np[a] = g.N[a] - 2;
    if (ps->np[a] % 2) {
      ins_set_error("spectral psolver: the number of volumes must be even in every direction (utils.jl:1-13)");
      delete ps;
      return INS_ERR_INVALID;
    }
    ps->kmax[a] = a == 0 ? ps->np[a] / 2 + 1 : ps->np[a];
    nreal *= ps->np[a];
    ncplx *= ps->kmax[a];
    om *= G->h[a];
  }
  bool ok = ps->pI.alloc(nreal) == INS_OK && ps->phat.alloc(ncplx) == INS_OK;
  for (int a = 0; ok && a < g.D; ++a) {  // âα(k) = 4 Ω sin²(π k / Npα) / Δxα², evaluated in double, stored in float
    std::vector<float> h(ps->kmax[a]);
    for (int k = 0; k < ps->kmax[a]; ++k) {
      const double sn = std::sin(M_PI * (double)k / ps->np[a]);
      h[k] = (float)(4.0 * om * sn * sn / (G->h[a] * G->h[a]));
    }
    ok = ps->ahat[a].alloc_copy_host(h.size(), h.data()) == INS_OK;
  }
  if (ok) {
    hipfftResult r1, r2;
    if (g.D == 2) {
      r1 = hipfftPlan2d(&ps->fwd, ps->np[1], ps->np[0], HIPFFT_R2C);
      r2 = r1 == HIPFFT_SUCCESS ? hipfftPlan2d(&ps->inv, ps->np[1], ps->np[0], HIPFFT_C2R) : r1;
    } else {
      r1 = hipfftPlan3d(&ps->fwd, ps->np[2], ps->np[1], ps->np[0], HIPFFT_R2C);
      r2 = r1 == HIPFFT_SUCCESS ? hipfftPlan3d(&ps->inv, ps->np[2], ps->np[1], ps->np[0], HIPFFT_C2R) : r1;
    }
    if (r1 == HIPFFT_SUCCESS && r2 != HIPFFT_SUCCESS) (void)hipfftDestroy(ps->fwd);
    ps->plans = r1 == HIPFFT_SUCCESS && r2 == HIPFFT_SUCCESS;
    ok = ps->plans;
  }
  if (!ok) {
    ins_set_error("ins_poisson_spectral_create_f32: allocation or hipFFT plan creation failed");
    ins_poisson_destroy_f32(ps);
    return INS_ERR_FFT;
  }
  // the plans above serve every route (ins_poisson_solve_f32); a route that cannot be set up leaves the solver one route down
  const F32Route want = ins_f32_choose(g.D, ps->np[0], ps->np[1], ps->np[2]);
  if (want != F32_HIPFFT && ins_poisson_spectral_create(G, &ps->ps64) == INS_OK) ps->route = F32_FP64_SPECTRA;  // the fused fp64 passes for project!
  if (want == F32_FLOAT2_SPECTRA && ps->route == F32_FP64_SPECTRA) {
    ps->kxs32 = (ps->kmax[0] + 15) & ~15;  // rows of the float2 spectrum padded to whole 128-B lines
    bool ok32 = ps->phat32.alloc_zero((size_t)ps->kxs32 * ps->np[1] * ps->np[2] * 2) == INS_OK;
    for (int a = 0; ok32 && a < 3; ++a) ok32 = ins_zsolve_twiddles_f32(ps->np[a], &ps->tw32[a]) == INS_OK;
    if (ok32) ps->route = F32_FLOAT2_SPECTRA;
  }
  *out = ps;
  return INS_OK;
}

static int solve32(ins_poisson32* ps, hipStream_t s) {  // pI -> pI
  const GridDev& g = ps->grid->g;
  INS_FFT_TRY(hipfftSetStream(ps->fwd, s));
  INS_FFT_TRY(hipfftSetStream(ps->inv, s));
  INS_FFT_TRY(hipfftExecR2C(ps->fwd, ps->pI, ps->phat));
  const float inv_n = 1.0f / ((float)ps->np[0] * (float)ps->np[1] * (float)ps->np[2]);
  const dim3 grid(cdiv(ps->kmax[0], 64), cdiv(ps->kmax[1], 4), g.D == 3 ? ps->kmax[2] : 1);
  K32_LAUNCH_BY_DIM(g.D, k32_symbol, grid, s, ps->phat, ps->ahat[0], ps->ahat[1], ps->ahat[2], ps->kmax[0], ps->kmax[1], inv_n);  // 2-D: ahat[2] is null
  INS_LAUNCH_CHECK();
  INS_FFT_TRY(hipfftExecC2R(ps->inv, ps->phat, ps->pI));
  return INS_OK;
}

// project!(u, setup; psolver, p) with T = Float32                                        pressure.jl:69-82
// u needs no valid ghosts on entry (periodic images are read); on return u and p carry their periodic ghosts.
extern "C" int ins_project_f32(const ins_grid_t* G, ins_poisson32_t* ps, float* u, float* p, void* stream) {
  INS_REQUIRE(G && ps && u && p, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  hipStream_t s = as_stream(stream);
  const Box32 b = box_of(G);
  const bool one_kernel = !ins_opt(OPT_INS_F32_SPLIT_GRADIENT);  // read per call; the own passes exist in 3-D only
  int rc;
  switch (ps->route) {
    case F32_WRAP: return ins_k32g_project(G, ps->wrap64, ps->p64, u, p, s);
    case F32_FLOAT2_SPECTRA:
      if ((rc = ins_k_spectral_solve_f32(ps->ps64, u, ps->pI, ps->phat32, ps->kxs32, ps->tw32[0], ps->tw32[1], ps->tw32[2], s))) return rc;
      return project_tail(G, b, u, p, (const float*)ps->pI, one_kernel, s);
    case F32_FP64_SPECTRA:
      if ((rc = ins_k_spectral_solve_from_u32(ps->ps64, u, s))) return rc;
      return project_tail(G, b, u, p, ins_k_spectral_pI(ps->ps64), one_kernel, s);
    case F32_HIPFFT:
      K32_LAUNCH_BY_DIM(b.D, k32_div, grid_over(b, false), s, b, u, ps->pI);
      INS_LAUNCH_CHECK();
      if ((rc = solve32(ps, s))) return rc;
      return project_tail(G, b, u, p, (const float*)ps->pI, false, s);  // the three kernels, in 3-D too
  }
  return INS_ERR_INVALID;
}

// psolver(p): solve L p = f on view(p, Ip) in place (pressure.jl:318-350); ghosts of p are refreshed
extern "C" int ins_poisson_solve_f32(ins_poisson32_t* ps, float* p, void* stream) {
  INS_REQUIRE(ps && p, "null argument");
  hipStream_t s = as_stream(stream);
  const ins_grid* G = ps->grid;
  const GridDev& g = G->g;
  if (ps->route == F32_WRAP) return ins_k32g_solve(G, ps->wrap64, ps->p64, p, s);
  // every spectral route: strip the ghosts (2-D copies), solve on the hipFFT plans, pad
  const size_t w = (size_t)ps->np[0] * sizeof(float);
  hipMemcpy3DParms c = {};
  c.srcPtr = make_hipPitchedPtr(p, (size_t)g.N[0] * sizeof(float), g.N[0], g.N[1]);
  c.srcPos = make_hipPos(sizeof(float), 1, g.D == 3 ? 1 : 0);
  c.dstPtr = make_hipPitchedPtr(ps->pI, w, ps->np[0], ps->np[1]);
  c.extent = make_hipExtent(w, ps->np[1], g.D == 3 ? ps->np[2] : 1);
  c.kind = hipMemcpyDeviceToDevice;
  INS_HIP_TRY(hipMemcpy3DAsync(&c, s));
  int rc = solve32(ps, s);
  if (rc) return rc;
  pad32(box_of(G), (const float*)ps->pI, p, s);
  INS_LAUNCH_CHECK();
  return INS_OK;
}

// ---------------------------------------------------------------------------------------------- explicit Runge-Kutta, T = Float32
extern "C" int ins_rk_destroy_f32(ins_rk32_t* rk) {
  delete rk;
  return INS_OK;
}

extern "C" int ins_rk_create_f32(const ins_grid_t* G, ins_poisson32_t* ps, int nstage, const double* A, const double* c, ins_rk32_t** out) {
  INS_REQUIRE(G && ps && A && c && out, "null argument");
  INS_REQUIRE(ps->grid == G, "psolver was created for a different grid");
  INS_REQUIRE(nstage >= 1 && nstage <= INS_MAX_STAGES, "unsupported number of stages");
  ins_rk32* rk = new ins_rk32();
  rk->grid = G;
  rk->ps = ps;
  rk->nstage = nstage;
  rk->A.assign(A, A + nstage * nstage);
  rk->c.assign(c, c + nstage);
  const size_t nvec = (size_t)G->ncell * G->g.D;
  rk->ku.resize(nstage);
  int rc = rk->p.alloc_zero(G->ncell);
  for (int i = 0; rc == INS_OK && i < nstage; ++i) rc = rk->ku[i].alloc_zero(nvec);
  for (int b = 0; rc == INS_OK && b < 2; ++b) rc = rk->ub[b].alloc_zero(nvec);
  if (rc != INS_OK) {
    ins_rk_destroy_f32(rk);
    return rc;
  }
  *out = rk;
  return INS_OK;
}

// Which stage loop a step takes: the only place these conditions are written.  Evaluated per call, since INS_DISABLE_INKERNEL_CORR, INS_RK_KEEP_K and
// INS_DISABLE_STEP_CHAIN are read per call; the solver's route is the one its creation stored.  (ins_dbg_rk32_route: the bools in this order, bit 0 up.)
struct Rk32Route {
  F32Route solver;
  bool general;         // walls / stretched spacings: the operator kernels of ins_f32g.hip, the reference's sequence stage by stage
  bool wide;            // the 64-wide stage kernel, the stage combination as its epilogue
  bool incorr;          // stages >= 2 correct the previous stage's velocity in registers: wide boxes on the fp64 solver's own passes (either spectra)
  bool float2_spectra;  // the solver's float pI is what the next stage's stencil kernel reads
  bool vbasis;          // stage-velocity basis: no stage force is stored or read
  bool chainable;       // ins_rk_steps_f32 folds a step's last correction into the next step's first stage
};
static Rk32Route rk32_route(const ins_rk32* rk) {
  const ins_grid* G = rk->grid;
  Rk32Route r;
  r.solver = rk->ps->route;
  r.general = !periodic_uniform(G);
  r.wide = !r.general && ins_flux64_supported(G);
  r.float2_spectra = r.solver == F32_FLOAT2_SPECTRA;
  r.incorr = r.wide && (r.float2_spectra || r.solver == F32_FP64_SPECTRA) && rk->nstage > 1 && G->uniform_exact && G->g.N[0] >= 8 && G->g.N[1] >= 8 &&
             G->g.N[2] >= 8 && !ins_opt(OPT_INS_DISABLE_INKERNEL_CORR);
  r.vbasis = r.incorr && !ins_opt(OPT_INS_RK_KEEP_K) && ins_rk_vbasis_possible(rk->A.data(), rk->nstage);
  r.chainable = r.float2_spectra && r.vbasis && !ins_opt(OPT_INS_DISABLE_STEP_CHAIN);  // the chain needs the solver's float pI and the stage-velocity basis
  return r;
}

// timestep!(method, stepper, Δt; cache) for closure_model = temp = bodyforce = nothing, T = Float32       step_explicit_runge_kutta.jl:4-59
// The caller's u is ustart for the whole step; on wide 3-D boxes the stage combination is the stencil kernel's epilogue.  As on the fp64 path (csrc/ins_rk.hip):
//   * stage-velocity basis: with in-register correction the uncorrected stage velocities stay in memory anyway, so the combination is written in terms of them
//     (V_i = (1 - Σβ) ustart + Σ β_im V_m + Δt A[i,i] k_i) and no stage force is stored or read — the `ku` arrays hold the stage velocities;
//   * chain bit 1: `u` holds the previous step's UNCORRECTED last stage velocity and the solver's pI its pressure: the first stage corrects in registers and
//     stores the corrected field as this step's ustart; bit 2: the last stage only solves (the next step of the chain corrects).
static int rk32_step(ins_rk32* rk, float visc, float* u, float dt, hipStream_t s, int chain) {
  const ins_grid* G = rk->grid;
  const int ns = rk->nstage, D = G->g.D;
  const long long nvec = G->ncell * D;
  const Rk32Route r = rk32_route(rk);
  const bool general = r.general, wide = r.wide, incorr = r.incorr, fl2 = r.float2_spectra, vbasis = r.vbasis;
  const bool raw_in = chain & 1, raw_out = chain & 2;
  int rc;
  if (general && r.solver != F32_WRAP) {
    ins_set_error("ins_rk_step_f32: this grid needs a solver made by ins_poisson_wrap_f32");
    return INS_ERR_UNSUPPORTED;
  }
  // F32_WRAP with !general (a wrapped solver on a periodic uniform box) takes the periodic loop without ghost fills: ADVICE.md, first finding, open
  if (!raw_in && (rc = general ? ins_k32g_apply_bc_u(G, u, s) : bc_periodic(G, u, D, s))) return rc;  // :19
  // Wide power-of-two boxes: the fp64 path's stage structure in float — stages >= 2 read the previous stage's UNCORRECTED u* and
  // its pressure and apply u = u* - ∇p in registers (CORR = 1), the solve forms Ω·div(u*) from the float field inside its x
  // pass; only the last stage materialises u (padded p, gradient-subtract, ghosts).
  const long long ncell_in = (long long)(G->g.N[0] - 2) * (G->g.N[1] - 2) * (G->g.N[2] - 2);
  if (incorr && !fl2 && !rk->pu && (rc = rk->pu.alloc(ncell_in))) return rc;
  const float* pcorr = fl2 ? rk->ps->pI : rk->pu;
  if (chain && !(incorr && fl2)) {
    ins_set_error("ins_rk_steps_f32: chained steps need the in-register correction on float2 spectra");
    return INS_ERR_UNSUPPORTED;
  }
  const float* cur = u;
  for (int i = 0; i < ns; ++i) {
    float* outp = (i == ns - 1 && ns > 1) ? u : (vbasis ? rk->ku[i] : rk->ub[i & 1]);
    if (wide) {
      // the V_m live in the ku arrays (float arrays behind RkEpi's untyped pointers: the kernels cast back); V_{i-1} is this stage's stencil input and the
      // kernel always has its uncorrected value in registers
      RkEpi epi = ins_rk_stage_terms(rk->A.data(), ns, i, (double)dt, rk->ku, (const float*)nullptr, vbasis ? RK_V_BASIS : RK_K_BASIS, true,
                                     RK_FORCE_DIAG_FIRST);
      epi.ustart = i == 0 ? nullptr : reinterpret_cast<const double*>(raw_in ? rk->ustart : u);
      epi.ustar = reinterpret_cast<double*>(outp);
      if (i == 0 && raw_in) epi.ustart_out = reinterpret_cast<double*>(rk->ustart.get());
      const bool corr = incorr && (i > 0 || raw_in);
      if ((rc = ins_k_flux64_f32(G, (double)visc, cur, vbasis ? rk->ub[0] : rk->ku[i], &epi, corr ? pcorr : nullptr, corr ? 1 : 0, s))) return rc;   // :21, :35-38
    } else {
      if ((rc = ins_momentum_f32(G, visc, cur, rk->ku[i], s))) return rc;       // :21
      float coef[INS_MAX_STAGES + 1];
      const float* k[INS_MAX_STAGES + 1];
      const int nt = ins_rk_sum_terms(rk->A.data(), ns, i, dt, rk->ku, (const float*)nullptr, coef, k);  // Δt (float)A[i,j], in float
      if ((rc = ins_k32_combine(nvec, u, outp, nt, coef, k, s))) return rc;      // :35-38
      if (general && (rc = ins_k32g_apply_bc_u(G, outp, s))) return rc;          // :47
    }
    if (incorr && (i < ns - 1 || raw_out) && fl2) {  // solve only, float2 spectra: p lands in the solver's float pI
      ins_poisson32* q = rk->ps;
      if ((rc = ins_k_spectral_solve_f32(q->ps64, outp, q->pI, q->phat32, q->kxs32, q->tw32[0], q->tw32[1], q->tw32[2], s))) return rc;
    } else if (incorr && i < ns - 1) {  // solve only: p (unpadded, float) for the next stage's in-register correction
      if ((rc = ins_k_spectral_solve_from_u32(rk->ps->ps64, outp, s))) return rc;
      hipLaunchKernelGGL(k32_cvt, dim3((unsigned)std::min<long long>((ncell_in + 255) / 256, 8192)), dim3(256), 0, s, ncell_in,
                         ins_k_spectral_pI(rk->ps->ps64), rk->pu);
      INS_LAUNCH_CHECK();
    } else if ((rc = ins_project_f32(G, rk->ps, outp, rk->p, s))) {             // :48-49 (periodic images: no ghost fill before)
      return rc;
    }
    if (general && (rc = ins_k32g_apply_bc_u(G, outp, s))) return rc;            // :49
    cur = outp;
  }
  if (ns == 1) INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], nvec * sizeof(float), hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

extern "C" int ins_rk_step_f32(ins_rk32_t* rk, float visc, float* u, float dt, void* stream) {
  INS_REQUIRE(rk && u, "null argument");
  return rk32_step(rk, visc, u, dt, as_stream(stream), 0);
}

// nsteps steps of size dt (the fixed-Δt loop of solve_unsteady, solver.jl:74-83) with the final correction of every step but the last folded into the next
// step's first stage kernel, as ins_rk_steps_f64; u is valid before and after the call.  Falls back to single steps where the chain does not apply.
extern "C" int ins_rk_steps_f32(ins_rk32_t* rk, float visc, float* u, float dt, int nsteps, void* stream) {
  INS_REQUIRE(rk && u && nsteps >= 0, "bad argument");
  const ins_grid* G = rk->grid;
  hipStream_t s = as_stream(stream);
  if (!rk32_route(rk).chainable || nsteps < 2) {
    for (int n = 0; n < nsteps; ++n) {
      int rc = rk32_step(rk, visc, u, dt, s, 0);
      if (rc) return rc;
    }
    return INS_OK;
  }
  if (!rk->ustart)
    if (int rc = rk->ustart.alloc((size_t)G->ncell * G->g.D)) return rc;
  for (int n = 0; n < nsteps; ++n) {
    int rc = rk32_step(rk, visc, u, dt, s, (n > 0 ? 1 : 0) | (n < nsteps - 1 ? 2 : 0));
    if (rc) return rc;
  }
  return INS_OK;
}

// ---------------------------------------------------------------------------------------------- explicit Runge-Kutta with the temperature equation
extern "C" int ins_rk_set_temperature_f32(ins_rk32_t* rk, const ins_temperature_desc_t* desc) {
  INS_REQUIRE(rk, "null argument");
  if (desc) {
    INS_REQUIRE(desc->gdir >= 0 && desc->gdir < rk->grid->g.D, "gdir out of range");
    rk->td = *desc;
  }
  rk->temp_on = desc != nullptr;
  return INS_OK;
}

// first use of a buffer: allocated and zeroed on the stream
static int zalloc32(DevBuf<float>* b, size_t bytes, hipStream_t s) { return *b ? INS_OK : b->alloc_zero_async(bytes / sizeof(float), s); }

// kind 0: no closure; 1: smagorinsky_closure(setup) with constant θ (operators.jl:1294-1305)
extern "C" int ins_rk_set_closure_f32(ins_rk32_t* rk, int32_t kind, float theta) {
  INS_REQUIRE(kind == 0 || kind == 1, "closure kind: 0 (none) or 1 (Smagorinsky)");
  INS_REQUIRE(rk, "null argument");
  rk->closure = kind;
  rk->theta = theta;
  return INS_OK;
}

// steady body force (setup.jl:25-32; operators.jl:873-880): a device vector field the caller keeps alive; NULL removes it
extern "C" int ins_rk_set_bodyforce_f32(ins_rk32_t* rk, const float* force) {
  INS_REQUIRE(rk, "null argument");
  rk->force = force;
  return INS_OK;
}

// timestep!(method, stepper, Δt; cache) with any of `temp`, a Smagorinsky closure and a steady body force, T = Float32       step_explicit_runge_kutta.jl:4-59
// Per stage: ku_i = momentum(u) + gravity(temp) + closure(u, θ) (:21, :31-34; operators.jl:873-880, 1294-1305) — the steady body force is not added to
// ku_i but rides in the combination as one more term (ins_rk_sum_terms); the closure force is formed in E, a field zeroed at its allocation of which only
// the degrees of freedom are ever written (one kernel where ins_smagforce_supported says so, else smagtensor! -> apply_bc_p! -> divoftensor!), and added
// to ku_i.  Then the temperature stage (:23-27, 39-44: one kernel, or operator by operator with INS_DISABLE_TEMP32_STAGE), the combination of u (:35-38),
// ghost fill, project!, ghost fill (:47-49) and the ghost fill of the new stage temperature, which is also the one the next stage (:19-20) or the end of
// the step (:55-56) asks for.  General grids run on the kernels of ins_f32g.hip and a wrapped solver, all-periodic uniform boxes (wide ones too) on
// ins_momentum_f32 / k32_combine / ins_project_f32; the temperature kernels are those of ins_temp32.hip on both.
// The caller's u is ustart for the whole step.  Stage temperatures alternate between the caller's array and one buffer so that the last stage lands in the
// caller's array; where that makes the first stage write it, that stage reads tempstart, a copy taken after the first ghost fill.
static int rk32_step_ext(ins_rk32* rk, float visc, float* u, float* temp, float dt, hipStream_t s) {
  const ins_grid* G = rk->grid;
  const GridDev& g = G->g;
  const int ns = rk->nstage, D = g.D;
  const long long nvec = G->ncell * D;
  const size_t sbytes = (size_t)G->ncell * sizeof(float);
  const Rk32Route r = rk32_route(rk);
  const bool general = r.general;
  const ins_temperature_desc_t& td = rk->td;
  const bool closure = rk->closure == 1;
  int rc;
  for (int a = 0; a < D; ++a)
    if (g.bc[a][0] == INS_BC_HALO || g.bc[a][1] == INS_BC_HALO) {
      ins_set_error("ins_rk_step_ext_f32: slab (halo) grids run in fp64 only");
      return INS_ERR_UNSUPPORTED;
    }
  if (general && r.solver != F32_WRAP) {
    ins_set_error("ins_rk_step_ext_f32: this grid needs a solver made by ins_poisson_wrap_f32");
    return INS_ERR_UNSUPPORTED;
  }
  if (temp) {
    if ((rc = zalloc32(&rk->tempstart, sbytes, s)) || (rc = zalloc32(&rk->tstage, sbytes, s))) return rc;
    if (td.dodissipation && (rc = zalloc32(&rk->diff, sbytes * D, s))) return rc;
    if ((int)rk->ktemp.size() < ns) rk->ktemp.resize(ns);
    for (int i = 0; i < ns; ++i)
      if ((rc = zalloc32(&rk->ktemp[i], sbytes, s))) return rc;
  }
  const bool smag1 = closure && ins_smagforce_supported(G);
  if (closure && (rc = zalloc32(&rk->E, sbytes * D, s))) return rc;
  if (closure && !smag1 && (rc = zalloc32(&rk->sigma, sbytes * (D * (D + 1) / 2), s))) return rc;
  float val[6];
  for (int q = 0; q < 6; ++q) val[q] = temp ? (float)td.val[q] : 0.f;
  auto bc_u = [&](float* v) { return general ? ins_k32g_apply_bc_u(G, v, s) : bc_periodic(G, v, D, s); };
  auto bc_temp = [&](float* t) { return ins_apply_bc_temp_f32(G, td.bc, val, t, s); };
  const bool one_pass = !ins_opt(OPT_INS_DISABLE_TEMP32_STAGE);
  const float a4 = (float)td.a4, a2 = (float)td.a2, dcoef = (float)td.diss_coef;

  if ((rc = bc_u(u))) return rc;                                                                           // :19
  const float* tin = nullptr;
  if (temp) {
    if ((rc = bc_temp(temp))) return rc;                                                                   // :20
    INS_HIP_TRY(hipMemcpyAsync(rk->tempstart, temp, sbytes, hipMemcpyDeviceToDevice, s));                  // state_copyto!(xstart, x)   :14
    tin = (ns & 1) ? rk->tempstart : temp;
  }
  const float* cur = u;
  for (int i = 0; i < ns; ++i) {
    float* outp = (i == ns - 1 && ns > 1) ? u : rk->ub[i & 1];
    float* tout = temp ? (((ns - 1 - i) & 1) ? rk->tstage : temp) : nullptr;
    if ((rc = ins_momentum_f32(G, visc, cur, rk->ku[i], s))) return rc;                                    // :21
    if (temp && (rc = ins_gravity_f32(G, td.gdir, a2, tin, rk->ku[i], s))) return rc;
    if (closure) {                                                                                         // :31-34
      if (smag1) {
        if ((rc = ins_k_smagforce_f32(G, rk->theta, cur, rk->E, s))) return rc;
      } else {
        if ((rc = ins_smagtensor_f32(G, rk->theta, cur, rk->sigma, s))) return rc;
        if ((rc = ins_k32g_apply_bc_p_fields(G, rk->sigma, D * (D + 1) / 2, s))) return rc;                // apply_bc_p!(σ, 0, setup)   operators.jl:1302
        if ((rc = ins_divoftensor_f32(G, rk->sigma, rk->E, s))) return rc;
      }
      hipLaunchKernelGGL(k32_add, dim3((unsigned)std::min<long long>((nvec + 255) / 256, 8192)), dim3(256), 0, s, nvec, rk->ku[i], (const float*)rk->E);
      INS_LAUNCH_CHECK();
    }
    if (temp) {
      float tcoef[INS_MAX_STAGES];
      const float* tk[INS_MAX_STAGES];
      for (int j = 0; j <= i; ++j) {
        tcoef[j] = dt * (float)rk->A[i * ns + j];
        tk[j] = rk->ktemp[j];
      }
      if (one_pass) {                                                                                      // :23-27, 39-44
        if (td.dodissipation && (rc = ins_k32t_diffusion(G, visc, cur, rk->diff, s))) return rc;
        const bool later = ins_rk_needed_later(rk->A.data(), ns, i);
        if ((rc = ins_k32t_stage(G, a4, dcoef, cur, tin, td.dodissipation ? rk->diff : nullptr, rk->tempstart, i, tcoef, tk, tcoef[i],
                                 later ? rk->ktemp[i] : nullptr, tout, s)))
          return rc;
      } else {
        INS_HIP_TRY(hipMemsetAsync(rk->ktemp[i], 0, sbytes, s));
        if ((rc = ins_convection_diffusion_temp_f32(G, a4, cur, tin, rk->ktemp[i], s))) return rc;
        if (td.dodissipation && (rc = ins_dissipation_f32(G, visc, dcoef, cur, rk->diff, rk->ktemp[i], s))) return rc;
        if ((rc = ins_k32_combine(G->ncell, rk->tempstart, tout, i + 1, tcoef, tk, s))) return rc;
      }
    }
    float coef[INS_MAX_STAGES + 1];
    const float* k[INS_MAX_STAGES + 1];
    const int nt = ins_rk_sum_terms(rk->A.data(), ns, i, dt, rk->ku, rk->force, coef, k);             // the body force: one more term
    if ((rc = ins_k32_combine(nvec, u, outp, nt, coef, k, s))) return rc;                                  // :35-38
    if (general && (rc = bc_u(outp))) return rc;                                                           // :47
    if ((rc = ins_project_f32(G, rk->ps, outp, rk->p, s))) return rc;                                      // :48-49 (periodic boxes: fills the ghosts itself)
    if (general && (rc = bc_u(outp))) return rc;
    if (temp && (rc = bc_temp(tout))) return rc;
    cur = outp;
    tin = tout;
  }
  if (ns == 1) INS_HIP_TRY(hipMemcpyAsync(u, rk->ub[0], nvec * sizeof(float), hipMemcpyDeviceToDevice, s));
  return INS_OK;
}

extern "C" int ins_rk_steps_ext_f32(ins_rk32_t* rk, float visc, float* u, float* temp, float dt, int nsteps, void* stream) {
  INS_REQUIRE(rk && u && nsteps >= 0, "null or bad argument");
  INS_REQUIRE(rk->temp_on == (temp != nullptr), "a temperature field needs ins_rk_set_temperature_f32 and vice versa");
  if (!temp && !rk->closure && !rk->force) return ins_rk_steps_f32(rk, visc, u, dt, nsteps, stream);  // the plain loop: fused stages, chained steps
  for (int n = 0; n < nsteps; ++n) {
    int rc = rk32_step_ext(rk, visc, u, temp, dt, as_stream(stream));
    if (rc) return rc;
  }
  return INS_OK;
}

extern "C" int ins_rk_step_ext_f32(ins_rk32_t* rk, float visc, float* u, float* temp, float dt, void* stream) {
  return ins_rk_steps_ext_f32(rk, visc, u, temp, dt, 1, stream);
}

// maximum(abs, divergence(u)) over Ip (diagnostic; blocking)                            operators.jl:106-125
extern "C" int ins_max_abs_divergence_f32(const ins_grid_t* G, ins_poisson32_t* ps, const float* u, float* out, void* stream) {
  INS_REQUIRE(G && ps && u && out, "null argument");
  hipStream_t s = as_stream(stream);
  int rc;
  if (ps->route == F32_WRAP) {  // any grid: divergence! on Ip of a padded scratch (zero elsewhere), maximum on the host
    if ((rc = ins_k32g_divergence(G, u, ps->div32, s))) return rc;
    return host_max_abs(ps->div32, G->ncell, s, out);
  }
  const Box32 b = box_of(G);  // every spectral route: Ω·div(u) in the solver's pI
  K32_LAUNCH_BY_DIM(b.D, k32_div, grid_over(b, false), s, b, u, ps->pI);
  INS_LAUNCH_CHECK();
  if ((rc = host_max_abs(ps->pI, (long long)ps->np[0] * ps->np[1] * ps->np[2], s, out))) return rc;
  *out /= b.om;
  return INS_OK;
}

// What csrc/ins_adjoint32.hip needs of a Float32 solver handle: the wrapped fp64 solver (nullptr: a spectral Float32 solver) with its padded fp64 scratch,
// and the grid the handle was made for.
ins_poisson* ins_k32_wrapped(const ins_poisson32* ps, double** p64) {
  *p64 = ps->p64;
  return ps->route == F32_WRAP ? ps->wrap64 : nullptr;
}
const ins_grid* ins_k32_solver_grid(const ins_poisson32* ps) { return ps->grid; }

// test hooks: the route a periodic uniform box would get under the current option values, without touching the device; a live integrator's solver route and
// the bit set of its step route (Rk32Route)
extern "C" int ins_dbg_f32_choose(int D, int n0, int n1, int n2) { return (int)ins_f32_choose(D, n0, n1, D == 3 ? n2 : 1); }
extern "C" int ins_dbg_rk32_route(const ins_rk32_t* rk, int32_t* flags) {
  const Rk32Route r = rk32_route(rk);
  if (flags) *flags = r.general | r.wide << 1 | r.incorr << 2 | r.float2_spectra << 3 | r.vbasis << 4 | r.chainable << 5;
  return (int)r.solver;
}
