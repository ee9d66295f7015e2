// Internal definitions shared by the HIP translation units of libinship.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ins_devbuf.h"
#include "ins_hip.h"

#define INS_EPS 2.220446049250313e-16
#define INS_MAX_STAGES 16

// ------------------------------------------------------------------------------------------------
// Error plumbing: every extern "C" entry returns an INS_ERR_* code and records a message.
// ------------------------------------------------------------------------------------------------
void ins_set_error(const char* fmt, ...);

#define INS_HIP_TRY(expr)                                                                   \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      ins_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));   \
      return INS_ERR_HIP;                                                                   \
    }                                                                                       \
  } while (0)

#define INS_FFT_TRY(expr)                                                         \
  do {                                                                            \
    hipfftResult _r = (expr);                                                     \
    if (_r != HIPFFT_SUCCESS) {                                                   \
      ins_set_error("%s:%d: %s -> hipfftResult %d", __FILE__, __LINE__, #expr, (int)_r); \
      return INS_ERR_FFT;                                                         \
    }                                                                             \
  } while (0)

#define INS_REQUIRE(cond, msg)                                        \
  do {                                                                \
    if (!(cond)) {                                                    \
      ins_set_error("%s:%d: %s (%s)", __FILE__, __LINE__, msg, #cond); \
      return INS_ERR_INVALID;                                         \
    }                                                                 \
  } while (0)

#define INS_LAUNCH_CHECK() INS_HIP_TRY(hipGetLastError())

// ------------------------------------------------------------------------------------------------
// Run-time switches (ins_options.hip): name = environment variable that initialises it = name accepted by ins_set_option.
// ------------------------------------------------------------------------------------------------
#define INS_OPT_LIST(X)          \
  X(INS_DISABLE_FAST3D)          \
  X(INS_K1_LDS)                  \
  X(INS_FLUX_ROWS)               \
  X(INS_FLUX_ZC)                 \
  X(INS_FLUX_XW)                 \
  X(INS_FLUX_BAR)                \
  X(INS_FLUX64_62_FROM)          \
  X(INS_DISABLE_FLUX128)         \
  X(INS_DISABLE_YZ_FUSED)        \
  X(INS_YZ_FUSED)                \
  X(INS_YZ_SKEL)                 \
  X(INS_YZ_PARTITIONS)           \
  X(INS_F32_ONE_COLUMN)          \
  X(INS_FLUX128_CORR)            \
  X(INS_FLUX128_XW)              \
  X(INS_FLUX128_ROWS)            \
  X(INS_FLUX128_ROWS_CORR)       \
  X(INS_FLUX128_NW)              \
  X(INS_FLUX128_ZC)              \
  X(INS_DISABLE_FDM_ZDCT)        \
  X(INS_DISABLE_FDM_ZFFT)        \
  X(INS_DISABLE_FDM_XFFT)        \
  X(INS_DISABLE_FDM_XYFFT)       \
  X(INS_DISABLE_OWNFFT)          \
  X(INS_OWNFFT_POW2_ONLY)        \
  X(INS_FIELDS_NO_MARCH)         \
  X(INS_FIELDS_ROWS)             \
  X(INS_FIELDS_NOBAR)            \
  X(INS_FIELDS_ZC)               \
  X(INS_DISABLE_FLUX2D)          \
  X(INS_DISABLE_FLUX64M)         \
  X(INS_DISABLE_SMAGFORCE)       \
  X(INS_DISABLE_SMAGFORCE_GEN)   \
  X(INS_SMAGFORCE_FORCE_GEN)     \
  X(INS_SMAGFORCE_ZC)            \
  X(INS_SMAGFORCE_BAR)         \
  X(INS_FLUX64M_ZC)              \
  X(INS_FLUX64M_NOBAR)           \
  X(INS_FLUX64M_XW)              \
  X(INS_FLUX64M_ROWS)            \
  X(INS_FLUX64M_SKIP_FIRST)      \
  X(INS_DISABLE_FLUX64)          \
  X(INS_FLUX64_ROWS)             \
  X(INS_FLUX64_ROWS_CORR)        \
  X(INS_FLUX64_ZC)               \
  X(INS_FLUX64_ZC_CORR)          \
  X(INS_FLUX64_XW)               \
  X(INS_FLUX64_LDS)              \
  X(INS_FLUX64_SKEL)             \
  X(INS_FLUX64_NW)               \
  X(INS_FLUX64_NT)               \
  X(INS_FLUX64_NOBAR)            \
  X(INS_FLUX64_MINTILES)         \
  X(INS_FLUX64_XW_CORR)          \
  X(INS_UNIFORM_BITWISE)         \
  X(INS_PHAT_DENSE)              \
  X(INS_DISABLE_FDM_FUSED)       \
  X(INS_DISABLE_FDM_FOLD)        \
  X(INS_DISABLE_FDM_UNFOLD4)     \
  X(INS_DISABLE_FDM_FOLDFUSE)    \
  X(INS_DISABLE_INKERNEL_CORR)   \
  X(INS_DISABLE_STAGE_RHS)       \
  X(INS_DISABLE_STAGE_XFWD)      \
  X(INS_DISABLE_STAGE_CARRY)     \
  X(INS_RK_KEEP_K)               \
  X(INS_DISABLE_EXT_FUSED)       \
  X(INS_EXT_TEMP_SPLIT)          \
  X(INS_DISABLE_FUSED_RK)        \
  X(INS_DISABLE_STEP_CHAIN)      \
  X(INS_DISABLE_STEP_GRAPH)      \
  X(INS_DISABLE_LINE3)           \
  X(INS_DISABLE_XYFUSED)         \
  X(INS_DISABLE_CORR2D)          \
  X(INS_SPECTRUM_ROCFFT)         \
  X(INS_X_SKEL)                  \
  X(INS_LINE3_TK)                \
  X(INS_LINE3_WGS)               \
  X(INS_STEP_GRAPH)              \
  X(INS_ZSOLVE_SKEL)             \
  X(INS_ZSOLVE_TK)               \
  X(INS_ZSOLVE_RADIX4)           \
  X(INS_ZSOLVE_NT)               \
  X(INS_ZSOLVE_WGS)              \
  X(INS_DISABLE_ZSOLVE)          \
  X(INS_ZTRI_SKEL)               \
  X(INS_CG_HOSTSYNC)             \
  X(INS_CG_BATCH)                \
  X(INS_F32_CORR_ROWS)           \
  X(INS_F32_FP64_SPECTRA)        \
  X(INS_F32_HIPFFT_PROJECT)      \
  X(INS_F32_SPLIT_GRADIENT)      \
  X(INS_DISABLE_TEMP32_STAGE)    \
  X(INS_FFT_ALLOW_RESET)         \
  X(INS_DISABLE_ADJ_TILED)     \
  X(INS_ADJ_STAGE_FUSED)       \
  X(INS_DISABLE_FILTER_TILED)
#define INS_OPT_ENUM(id) OPT_##id,
enum InsOptId { INS_OPT_LIST(INS_OPT_ENUM) INS_OPT_COUNT };
#undef INS_OPT_ENUM
long long ins_opt(int id);  // current value (0 = off / default)
long long ins_opt_epoch();  // bumped by every ins_set_option: cached launch plans (step graphs) are rebuilt when it moves

// ------------------------------------------------------------------------------------------------
// Device view of the grid, passed to kernels by value (lives in the kernarg segment -> SGPR loads).
// Metric tables are tiny 1-D device vectors (<= 4 KB each), L1/L2/K$-resident.
//   rdx  = 1/Δ      rdxu = 1/Δu        (reciprocal tables: the reference's 27 fp64 divisions per cell
//   mdx  = Δ  > 2eps ? 1/Δ  : 0         become multiplies; <= 1 ulp per term, inside the 1e-12 tolerance)
//   mdxu = Δu > 2eps ? 1/Δu : 0        (the `(Δ > 2eps) * ∂` strong-zero masks of operators.jl:683-684)
// ------------------------------------------------------------------------------------------------
struct GridDev {
  int D;
  int N[3];
  long long sx[3];  // element strides of directions 0..2
  long long sc;     // component stride = prod(N)
  const double* dx[3];
  const double* dxu[3];
  const double* rdx[3];
  const double* rdxu[3];
  const double* mdx[3];
  const double* mdxu[3];
  const double* A1[3][3];
  const double* A2[3][3];
  int iu_lo[3][3], iu_hi[3][3];
  int ip_lo[3], ip_hi[3];
  int bc[3][2];
  double bc_u[3][2][3];
};

struct ins_grid {
  ins_grid_desc_t desc;  // host copy (metric pointers below are re-pointed to `host`)
  std::vector<double> host;
  DevBuf<double> dev;  // one device slab holding every table
  GridDev g;
  bool all_periodic = false;
  bool uniform = false;
  double h[3] = {0, 0, 0};  // Δx[α] of the first volume (uniform grids)
  long long ncell = 0;      // prod(N)
  bool all_dof = false;        // every interior volume is a DOF of every component (all-periodic)
  bool uniform_exact = false;  // all metric records bitwise identical over the used index range
  DevBuf<unsigned char> rec_dev;  // flux-kernel metric records (ins_fast3d_flux.hip), built lazily
  double rec_visc = -1.0;
  DevBuf<unsigned char> rec_diff_dev;  // the same records with zero interpolation weights: the flux kernels then evaluate diffusion!(F, u) alone
  double rec_diff_visc = -1.0;
  // scratch for blocking reductions
  DevBuf<double> red_dev;
  HostPinned<double> red_host;
  // ∇ubar of the tensor-basis pullbacks (ins_tensorclosure.hip): D·D scalar fields, allocated on first use
  DevBuf<double> gradbar_dev;
  // workgroup partials of the Smagorinsky force pullback's θ cotangent (ins_smagpullback.hip), allocated on first use
  DevBuf<double> smagpart_dev;
};

enum PoissonKind { POISSON_SPECTRAL = 0, POISSON_CG = 1, POISSON_FDM = 2 };

// fast-diagonalisation direct solver (ins_fdm.hip)
struct ins_fdm;
int ins_fdm_create(int D, const int n[3], const double* const V[3], const double* const lam[3], int singular, ins_fdm** out);
int ins_fdm_destroy(ins_fdm* F);
int ins_fdm_enable_zfft(ins_fdm* F, double hz, const double* lam_z_host);
int ins_fdm_enable_zdct(ins_fdm* F, double hz, const double* lam_z_host);
int ins_fdm_enable_xfft(ins_fdm* F, double hx, const double* lam_x_host);
int ins_fdm_enable_xyfft(ins_fdm* F, double hx, double hy, const double* lam_x_host, const double* lam_y_host);
int ins_fdm_solve(ins_fdm* F, hipStream_t s, const ins_grid* G = nullptr, const double* u = nullptr, bool folded_io = false);
int ins_fdm_fold_mask(const ins_fdm* F);  // which directions run as folded half-size GEMMs (bit a = direction a)
int ins_fdm_modes(const ins_fdm* F);      // which directions run in trigonometric modes (1 Fourier z, 2 Fourier x, 4 Fourier x and y, 8 cosine z)
bool ins_fdm_takes_u(const ins_fdm* F);
double* ins_fdm_buffer(ins_fdm* F);
const double* ins_fdm_mean(ins_fdm* F);  // device scalar the consumer subtracts (singular systems), or nullptr

// Launch sequence of a spectral solver: chosen once, when the solver is created (ins_spectral_choose, ins_poisson.hip), and dispatched on everywhere.
enum SpectralRoute {
  ROUTE_ROCFFT = 0,     // rocFFT plans over all D directions + k_symbol
  ROUTE_ROCFFT_ZFUSED,  // 3-D: batched rocFFT (x,y) plans + the fused z kernel (ins_zsolve.hip)
  ROUTE_OWN2D,          // 2-D: own x forward, the fused solve kernel along y, own x inverse
  ROUTE_OWN2D_ONE,      // 2-D, up to 64 x 64 volumes: the whole solve as one launch (k_xysolve2d)
  ROUTE_OWN_LDS,        // 3-D: own x, LDS y (k_yfft), fused z, y, x
  ROUTE_OWN_LINE3,      // 3-D: the same with the y passes on the register passes (k_line3, ins_zsolve.hip)
  ROUTE_OWN_XY,         // 3-D, planes of 16 .. 64 on both sides: xy forward, fused z, xy inverse (k_xy*)
  ROUTE_OWN_YZ,         // 3-D, opt-in: own x, the z direction riding on the two LDS y passes (k_yz_*), own x: four passes
};
// Storage order in which a route's y pass leaves ky; ahat[1] is uploaded in that order, and nowhere else does the order enter.
enum KyOrder { KY_NATURAL = 0, KY_DIGITREV, KY_LINE3 };  // rocFFT and the 2-D kernels / the LDS passes and k_xy / k_line3

struct ins_poisson {
  PoissonKind kind;
  const ins_grid* grid;  // borrowed
  // spectral
  hipfftHandle plan_fwd = 0, plan_inv = 0;
  SpectralRoute route = ROUTE_ROCFFT;
  KyOrder ky_order = KY_NATURAL;
  DevBuf<double> pI;               // real n^D
  DevBuf<double> rhs;              // real n^D, allocated on first use: Ω·div(u*) written by the stage kernel (ins_poisson_stage_rhs; pI is that kernel's pressure input)
  DevBuf<hipfftDoubleComplex> phat;     // (n/2+1) n [n]
  DevBuf<double> ahat[3];
  int np[3] = {1, 1, 1};
  int kmax[3] = {1, 1, 1};
  hipStream_t plan_stream = nullptr;
  int kxs = 0;              // own routes: row stride of phat (kmax[0] rounded up to 8 complex = 128 B)
  bool spec_pending = false;  // a stage kernel has been handed phat for the x-spectrum of its right-hand side (ins_poisson_stage_spec) and no solve has consumed it yet
  DevBuf<double> tw;        // z twiddles
  DevBuf<double> tw_x;      // x / y twiddles (own routes)
  DevBuf<double> tw_y;
  int yz_P = 0;             // ROUTE_OWN_YZ: partition count of the k_yz_* passes; 0 on every other route
  DevBuf<double> yz_scratch;
  // cg
  double abstol = 0, reltol = 0;
  long long maxiter = 0;
  DevBuf<double> r, L, q, dinv;
  bool bordered = false;
  bool singular = true;  // no PressureBC side
  long long ndof = 0;
  long long last_iter = 0;
  double last_res = 0;
  DevBuf<double> cg_scal;     // device scalars + block partials of the device-resident iteration
  HostPinned<double> cg_host;  // pinned mirror of the scalars
  struct ins_comm* comm = nullptr;  // borrowed; z-slab CG: scalar all-reduces + ghost planes of q (ins_poisson_cg_set_comm)
  // fdm (psolver_direct)
  ins_fdm* fdm = nullptr;  // owned: ins_fdm_destroy
};

struct ins_rk_ext;  // temperature equation / closure state of the extended stage loop (ins_rk_ext.hip)
void ins_rk_ext_free(ins_rk_ext* e);
struct ins_rk {
  const ins_grid* grid;  // borrowed
  ins_poisson* ps;       // borrowed
  int nstage;
  std::vector<double> A, c;
  DevBuf<double> ustart;
  std::vector<DevBuf<double>> ku;
  DevBuf<double> p;
  DevBuf<double> ub[2];  // ping-pong stage velocities of the fused path
  std::vector<double*> vb;  // borrowed: all uncorrected stage velocities V_0..V_{s-2} (stage-velocity basis, ins_rk.hip); ub[0], ub[1], then vb_extra
  std::vector<DevBuf<double>> vb_extra;  // the arrays of vb beyond ub[0..1]
  const double* force = nullptr;  // borrowed: steady body force field, ins_rk_set_bodyforce
  ins_rk_ext* ext = nullptr;
  long long stage_carry_launches = 0;  // stage kernels enqueued that stored a carried combination (ins_dbg_stage_carry_used)
  long long stage_rhs_launches = 0;  // stage kernels enqueued that wrote the Poisson right-hand side themselves (ins_dbg_stage_rhs_used)
  long long stage_xfwd_launches = 0;  // those of them that stored its x-spectrum instead of the real-space array (ins_dbg_stage_xfwd_used)
  bool profiling = false;
  std::vector<hipEvent_t> prof_events;  // (start, stop) pairs around momentum launches
  void* step_graph = nullptr;           // launch-bound boxes: one step of ins_rk_steps_f64 captured as a hipGraph (ins_rk.hip)
};

// Metric records of the flux-form stage kernels on stretched / masked grids (ins_fast3d_flux.hip builds them per viscosity: ins_flux3d_prepare;
// ins_flux64m.hip reads the same tables).  One record per (direction d, index idx); 16 doubles = 128 B so a record is one aligned scalar burst.
//   vs = ν·mdx[d][idx+1]   diffusion coefficient of the upper d-face for the d-component   (Δb, α == β)
//   vo = ν·mdxu[d][idx]    ... for the other components                                     (Δb, α != β)
//   a[β], b[β] = ½A₂[β][d][idx], ½A₁[β][d][idx+1]   half weights of component β read along d
//   rs = 1/Δu[d][idx], ro = 1/Δ[d][idx]              control-volume width reciprocals (α == β / α != β)
struct Rec {
  double vs, vo, a0, b0, a1, b1, a2, b2, rs, ro, pad[6];
};

// Runge-Kutta stage epilogue fused behind the stencil (K1 + K6): with f = momentum(u) still in registers,
//   u* = ustart + Σ_j (Δt A[i,j]) k_j + (Δt A[i,i]) f          (step_explicit_runge_kutta.jl:35-38, same order)
// is written in the same pass, and k_i = f is stored only when a later stage needs it.
struct RkEpi {
  int n;                    // previous-stage terms with non-zero coefficient
  int write_k;              // store k_i
  double coef[INS_MAX_STAGES + 1];  // + 1: the steady body force is one more term (ins_rk_set_bodyforce)
  const double* k[INS_MAX_STAGES + 1];
  double coef_self;         // Δt A[i,i]
  double self_in;           // coefficient of the stencil input itself (its uncorrected value, taken from registers: ins_flux64.hip)
  double c0m1;              // ustart enters as (1 + c0m1)·ustart; 0 in the k-basis, -Σ coef in the stage-velocity basis (ins_rk.hip)
  const double* ustart;     // the array the combination starts from, as (1 + c0m1)·ustart: the step's start velocity, or (c0m1 == 0) the combination S an
                            // earlier stage carried forward (carry_out below).  nullptr: it starts from the stencil input itself (first stage)
  double* ustar;            // stage velocity out (interior volumes only)
  double* ustart_out;       // optional (first stage of a chained step, ustart == nullptr): the corrected stencil input is stored here
  double* carry_out;        // optional (ins_flux64_stage_carry_supported; ins_rk_terms.h, RkCarryPlan): S = ca[0]·s + ca[1]·(the uncorrected stencil input) +
                            // ca[2]·u* is stored here, s = the combination before coef_self·f is added.  An array no input of the launch lives in
  double ca[3];
  double* rhs_out;          // optional (ins_flux64_stage_rhs_supported): Ω·div(u*) of the stored stage velocity, unpadded n^3 (never the pressure input pI)
  double* spec_out;         // optional (ins_flux64_stage_xfwd_supported; instead of rhs_out): the half-complex x-spectrum of that right-hand side, the layout k_xfwd
                            // writes (kx 0 .. n0/2 natural, spec_kxs complex per row), into the solver's phat; spec_tw: the x twiddle table (n0 complex)
  const double* spec_tw;
  int spec_kxs;
  const double* extra;      // optional vector field added to the stage force before it is used and stored (closure term: ins_rk_ext.hip)
  const double* gtemp;      // optional temperature field: gravity! is added to component gdir of the stage force (ga2 = α2)
  double ga2;
  int gdir;
  double* wout;             // optional: w_α = u_α · diffusion(u)_α of the stencil input is stored here (dissipation!, ins_rk_ext.hip)
  const struct TempEpi* tstage;  // optional (HOST pointer, read at launch): the temperature equation's stage inside the stage kernel
};

// The stage kernel stores u* over an array it also reads (its stencil input `in`, ustart or a stage term): safe cell by cell, but not for a kernel that reads
// neighbouring cells of its epilogue inputs (epi.rhs_out), which another workgroup may already have overwritten.
static inline bool ins_stage_out_aliases_input(const RkEpi& epi, const void* in) {
  bool a = (const void*)epi.ustar == in || epi.ustar == epi.ustart;
  for (int q = 0; q < epi.n; ++q) a = a || epi.ustar == epi.k[q];
  return a;
}
// The carried combination goes to an array of its own: other workgroups still read the halo rows and planes of the stencil input, and u* must not land on it.
static inline bool ins_stage_carry_aliases(const RkEpi& epi, const void* in) {
  bool a = (const void*)epi.carry_out == in || epi.carry_out == epi.ustart || epi.carry_out == epi.ustar;
  for (int q = 0; q < epi.n; ++q) a = a || epi.carry_out == epi.k[q];
  return a;
}

// One stage of the temperature equation carried by the 64-wide stage kernel (ins_flux64.hip, EXTRA; step_explicit_runge_kutta.jl:23-27, 39-44):
//   ktemp_i = convection_diffusion_temp(u, temp) + dissipation(u),   temp_out = tempstart + Σ_j coef_j k_j + c_self ktemp_i
struct TempEpi {
  const double* temp;       // T_i, padded, ghost volumes valid
  const double* tempstart;
  double* temp_out;         // T_{i+1}: another array than temp
  double* ktemp_out;        // nullable
  int n;
  double coef[INS_MAX_STAGES];
  const double* k[INS_MAX_STAGES];
  double c_self, a4, dcoef;  // Δt A[i,i];  α4;  Re·α1/γ (0: no dissipation term)
};


// ------------------------------------------------------------------------------------------------
// Internal launchers (stream-ordered, non-blocking) used across translation units.
// ------------------------------------------------------------------------------------------------
int ins_k_apply_bc_u(const ins_grid* grid, double* u, int dudt, const double* const* planes, hipStream_t s);
int ins_k_apply_bc_p(const ins_grid* grid, double* p, hipStream_t s);
int ins_k_apply_bc_p_fields(const ins_grid* grid, double* p, int nf, hipStream_t s);
int ins_k_momentum(const ins_grid* grid, double visc, const double* u, double* F, hipStream_t s);
// ins_operators.hip: momentum! on any grid, one volume per work-item
int ins_k_momentum_generic(const ins_grid* G, double visc, const double* u, double* F, hipStream_t s);
// ins_fast3d.hip: momentum! on the tiled 3-D kernels (ins_fast3d_supported); zero_shell: also zero the ghost shell of F
int ins_k_momentum_fast3d(const ins_grid* G, double visc, const double* u, double* F, hipStream_t s);
int ins_k_momentum_fast3d_opts(const ins_grid* G, double visc, const double* u, double* F, bool zero_shell, hipStream_t s);
// ins_fast3d_flux.hip: the flux-form kernels' metric records for this viscosity (struct Rec), built on first use; momentum!; fill!(F, 0) + diffusion!(F, u)
int ins_flux3d_prepare(const ins_grid* G, double visc, hipStream_t s);
int ins_k_momentum_flux3d(const ins_grid* G, double visc, const double* u, double* F, bool zero_shell, hipStream_t s);
int ins_k_diffusion_flux3d(const ins_grid* G, double visc, const double* u, double* F, bool zero_shell, hipStream_t s);
// ins_flux64.hip: the 64-outputs-per-wavefront stage kernel for periodic, exactly-uniform 3-D boxes; corr_mode != 0: u is uncorrected, pI its pressure
bool ins_flux64_supported(const ins_grid* G);
int ins_k_flux64(const ins_grid* G, double visc, const double* u, double* F, const RkEpi* epi, const double* pI, int corr_mode, hipStream_t s, int part = 0);
// ins_flux64m.hip: the same width on stretched / masked grids; p_padded != nullptr: u is the previous stage's uncorrected u* (boundary data applied)
bool ins_flux64m_supported(const ins_grid* G);
int ins_k_flux64m(const ins_grid* G, double visc, const double* u, double* k_out, const RkEpi& epi, const double* p_padded, hipStream_t s);
// ins_flux128.hip: two x-columns per lane wherever the box allows it (ins_k_flux64 dispatches to it)
bool ins_flux128_supported(const ins_grid* G, const RkEpi* epi, int corr_mode, bool f32);
int ins_k_flux128(const ins_grid* G, double visc, const double* u, double* F, const RkEpi* epi, const double* pI, int corr_mode, hipStream_t s, int part);
int ins_k_divergence(const ins_grid* grid, const double* u, double* div, hipStream_t s);
int ins_k_diffusion_overwrite(const ins_grid* grid, double visc, const double* u, double* F, hipStream_t s);
int ins_k_scalewithvolume(const ins_grid* grid, double* p, hipStream_t s);
int ins_k_applypressure(const ins_grid* grid, double* u, const double* p, hipStream_t s);
int ins_k_laplacian(const ins_grid* grid, const double* p, double* L, hipStream_t s);
int ins_k_project(const ins_grid* grid, ins_poisson* ps, double* u, double* p, hipStream_t s);
int ins_k_momentum_rk_fused(const ins_grid* G, double visc, const double* u_in, double* k_out, const RkEpi& epi, hipStream_t s);
bool ins_flux2d_supported(const ins_grid* G);
int ins_k_flux2d(const ins_grid* G, double visc, const double* u, double* F, const RkEpi* epi, hipStream_t s, const double* pI = nullptr);
int ins_k_project_periodic_solve_only_2d(const ins_grid* G, ins_poisson* ps, const double* u, hipStream_t s);
int ins_k_momentum_rk_fused_generic(const ins_grid* G, double visc, const double* u_in, double* k_out, const RkEpi& epi, hipStream_t s);
int ins_k_momentum_rk_fused_corr(const ins_grid* G, double visc, const double* ustar_prev, const double* pI, double* k_out, const RkEpi& epi,
                                 hipStream_t s);
int ins_k_momentum_rk_fused_corr_slab(const ins_grid* G, double visc, const double* ustar_prev, const double* p_ext, double* k_out,
                                      const RkEpi& epi, hipStream_t s, int part = 0);
bool ins_corr3_supported(const ins_grid* G);
int ins_k_momentum_rk_fused_corr3(const ins_grid* G, double visc, const double* ustar_prev, const double* p_padded, double* k_out, const RkEpi& epi,
                                  hipStream_t s);
bool ins_k_project_fdm_fused(const ins_poisson* ps);
int ins_k_project_fdm_solve_only(const ins_grid* G, ins_poisson* ps, const double* u, double* p, hipStream_t s);
int ins_k_project_periodic_fused_2d(const ins_grid* G, ins_poisson* ps, double* u, double* p, bool keep_p, hipStream_t s);
bool ins_poisson_own2d(const ins_poisson* ps);
bool ins_k_spectral_own3d(const ins_poisson* ps);  // 3-D spectral solver every pass of which is one of the library's own kernels
// project! of the fused periodic 3-D stage from interior values, ghost volumes filled; uout != nullptr: u stays and the corrected field goes to uout
int ins_k_project_periodic_fused(const ins_grid* G, ins_poisson* ps, double* u, double* p, bool keep_p, hipStream_t s, double* uout = nullptr,
                                 const double* rhs = nullptr, bool from_spec = false);
// rhs != nullptr (own-FFT routes): the right-hand side Ω·div(u) is already in that buffer (the stage kernel wrote it) and the x pass reads it instead of u
// from_spec: a stage kernel has stored the x-spectrum of the right-hand side in phat (ins_poisson_stage_spec): the solve starts at its y pass
int ins_k_project_periodic_solve_only(const ins_grid* G, ins_poisson* ps, const double* u, hipStream_t s, const double* rhs = nullptr, bool from_spec = false);
bool ins_flux64_stage_rhs_supported(const ins_grid* G, int corr_mode);  // the stage kernel of this box can write that right-hand side (ins_flux64.hip)
// ... and can store the x-forward transform of it instead, so the solve starts at its y pass (256-wide rows; ins_flux64.hip, XF)
bool ins_flux64_stage_xfwd_supported(const ins_grid* G, int corr_mode);
bool ins_flux64_stage_carry_supported(const ins_grid* G);            // its correcting stage kernel can store a carried combination (RkEpi::carry_out)
double* ins_poisson_stage_rhs(ins_poisson* ps);                        // its buffer (nullptr: no own-FFT 3-D route, or out of memory)
// The solver's spectrum buffer as the output of a stage kernel that reads `pI_in` as its pressure: phat, its row stride and the x twiddles.  nullptr: the solver's
// route does not begin with the separate x-forward pass, or phat is that kernel's input.  The next solve must be ins_k_project_periodic_solve_only(.., from_spec).
double* ins_poisson_stage_spec(ins_poisson* ps, const void* pI_in, const double** tw, int* kxs);
bool ins_poisson_stage_spec_possible(const ins_poisson* ps);
int ins_k_poisson_solve(ins_poisson* ps, double* p, hipStream_t s);
bool ins_fast3d_supported(const ins_grid* G);

// ins_fields.hip: one stage of the temperature equation (w, diff nullable; pI != nullptr: u is uncorrected); smagtensor! of u = ustar - ∇p formed in registers
int ins_k_temp_stage(const ins_grid* G, double a4, double coef, const double* u, const double* temp, const double* w, const double* tempstart, int n,
                     const double* coefs, const double* const* ks, double c_self, double* ktemp_out, double* temp_out, hipStream_t s, const double* pI,
                     const double* diff = nullptr);
int ins_k_smagtensor_corr(const ins_grid* G, double theta, const double* ustar, const double* pI, double* sig, hipStream_t s);
// ins_smagforce.hip: the Smagorinsky closure force in one kernel, and the grids it takes (both precisions).  pI != nullptr: u is an uncorrected stage velocity
bool ins_smagforce_supported(const ins_grid* G);
int ins_k_smagforce(const ins_grid* G, double theta, const double* u, const double* pI, double* sout, hipStream_t s);
// ins_tensorclosure.hip: the grid handle's ∇ubar scratch (D·D doubles per volume), allocated and grown on demand
int ins_k_gradbar_scratch(const ins_grid* G, double** out);
// ... and pass 2 of its pullbacks: ubar (+)= ∇ᵀ of the ∇ubar scratch gb, over the whole padded array
int ins_k_gradu_adjoint(const ins_grid* G, const double* gb, double* ubar, bool accumulate, hipStream_t s);
// ins_smagpullback.hip: the grid handle's scratch for the workgroup partials of the Smagorinsky force pullback (one double per workgroup of its pass 1)
int ins_k_smag_partials(const ins_grid* G, double** out);
// ins_adjoint.hip: transposes of apply_bc_u! / apply_bc_p! in place, and ubar = J(u)ᵀ (Σ_q coefs[q]·ks[q]) (the reverse Runge-Kutta stage)
int ins_k_apply_bc_u_pullback(const ins_grid* G, double* u, hipStream_t s);
int ins_k_apply_bc_p_pullback(const ins_grid* G, double* p, hipStream_t s);
int ins_k_momentum_pullback_comb(const ins_grid* G, double visc, const double* u, int nterms, const double* coefs, const double* const* ks, double* ubar,
                                 hipStream_t s);
// ins_ztri.hip: the z-slab solver's distributed tridiagonal passes over the line range [l_lo, l_lo + l_cnt) of the kxn·n1 lines, launched by ins_slab.hip
int ins_k_ztri_forward(double* work, int kxn, int kxs, int n1, int m, int nranks, int rank, const double* ax, const double* ay, double c,
                       double scale, double* edge, long long l_lo, long long l_cnt, hipStream_t s);
int ins_k_ztri_finish(double* work, int kxn, int kxs, int n1, int m, int nranks, int rank, const double* ax, const double* ay, double c,
                      const double* edges_all, long long stride, double* bc, long long l_lo, long long l_cnt, hipStream_t s);

// Which stage loop an integrator runs (ins_rk.hip, ins_rk_ext.hip).  Each is the whole condition; what only one caller asks in addition (time-dependent
// boundary planes, a body force, the closure / temperature state, the solver's own FFT passes) stands at that caller.
// fused periodic 3-D loop (rk_step_fused_periodic)
static inline bool ins_rk_fused3d(const ins_rk* rk) {
  const ins_grid* G = rk->grid;
  bool ok = !ins_opt(OPT_INS_DISABLE_FUSED_RK) && G->g.D == 3 && G->all_periodic && G->all_dof && rk->ps->kind == POISSON_SPECTRAL && ins_fast3d_supported(G);
  for (int a = 0; ok && a < 3; ++a) ok = rk->ps->np[a] >= 2;
  return ok;
}
// fused periodic 2-D loop (rk_step_fused_periodic_2d); both conditions imply a periodic box on the spectral solver
static inline bool ins_rk_fused2d(const ins_rk* rk) {
  return !ins_opt(OPT_INS_DISABLE_FUSED_RK) && rk->grid->g.D == 2 && ins_poisson_own2d(rk->ps) && ins_flux2d_supported(rk->grid);
}
// on those loops: stages >= 2 read the previous stage's uncorrected u* and its pressure and correct in registers
static inline bool ins_rk_inkernel3d(const ins_rk* rk) {
  const ins_grid* G = rk->grid;
  return !ins_opt(OPT_INS_DISABLE_INKERNEL_CORR) && G->uniform_exact && rk->nstage > 1 && G->g.N[0] >= 8 && G->g.N[1] >= 8 && G->g.N[2] >= 8;
}
static inline bool ins_rk_inkernel2d(const ins_rk* rk) {
  return rk->nstage > 1 && !ins_opt(OPT_INS_DISABLE_INKERNEL_CORR) && !ins_opt(OPT_INS_DISABLE_CORR2D) && rk->grid->g.N[0] >= 6 && rk->grid->g.N[1] >= 6;
}
// consecutive steps can hand their last correction to the next step's first stage kernel (ins_rk_steps_f64)
static inline bool ins_rk_chainable(const ins_rk* rk) {
  return !ins_opt(OPT_INS_DISABLE_STEP_CHAIN) && ((ins_rk_fused3d(rk) && ins_rk_inkernel3d(rk)) || (ins_rk_fused2d(rk) && ins_rk_inkernel2d(rk)));
}
// Ensemble stepping (ins_rk_ensemble.hip): the launchers of the chained 2-D loop with the member as one more launch dimension.  Member b of an operand
// lies b·(its stride) elements behind the pointer handed over; RkMemberStrides names the operands of the stage kernel (u: stencil input, p: its unpadded
// pressure, F: k_i out, then the RkEpi operands: ustart, every k[q], ustar, ustart_out).
struct RkMemberStrides {
  long long u, p, F, ustart, k, ustar, ustart_out;
};
int ins_k_flux2d_members(const ins_grid* G, double visc, const double* u, double* F, const RkEpi& epi, hipStream_t s, const double* pI, int nb,
                         const RkMemberStrides& st);
// its force form: F[b] = momentum!(u[b]), interior only (the projected right-hand side of all members, ins_rk_ensemble_rhs_f64)
int ins_k_flux2d_members_force(const ins_grid* G, double visc, const double* u, long long ustride, double* F, long long fstride, int nb, hipStream_t s);
int ins_k_solve_members_2d(const ins_grid* G, const ins_poisson* ps, const double* u, long long ustride, int nb, double* pI, double* phat, const double* zrows,
                           hipStream_t s);
int ins_k_grad_ghost_members_2d(const ins_grid* G, const ins_poisson* ps, double* u, long long ustride, int nb, const double* pI, hipStream_t s);
// the same pass with every ghost volume written as 0 instead of its periodic image: the last pass of the members' projection pullback (Rᵀ of E·P·R)
int ins_k_grad_zero_ghost_members_2d(const ins_grid* G, const ins_poisson* ps, double* u, long long ustride, int nb, const double* pI, hipStream_t s);
// ubar[b] (+)= J_F(u[b])ᵀ phi[b] on the whole padded array of every member, one launch (ins_adjoint.hip, k_momentum_pullback_members_2d)
int ins_k_momentum_pullback_members_2d(const ins_grid* G, double visc, const double* u, long long ustride, const double* phi, long long pstride, double* ubar,
                                       long long bstride, bool acc, int nb, hipStream_t s);
int ins_k_ownfft_xfwd_members(const ins_grid* G, const double* u, long long mstride, double* phat, int n0, int n1, int nb, const double* tw, hipStream_t s, int kxs);
int ins_k_ownfft_xinv_members(const double* phat, double* pI, int n0, int n1, int nb, const double* tw, hipStream_t s, int kxs);
// the x pass fed from the velocity components of all members (ghosts stripped in the load): phat holds [ky][2·member + component][kxs]
int ins_k_ownfft_xfwd_field_members(const ins_grid* G, const double* u, long long mstride, double* phat, int n0, int n1, int nb, const double* tw, hipStream_t s,
                                    int kxs);
// The ensemble handle (ins_rk_ensemble.hip); the observers of ins_rk_ensemble_observe.hip keep their workgroup partials on it.
struct ins_rk_ensemble {
  const ins_grid* grid = nullptr;  // borrowed
  ins_poisson* ps = nullptr;       // borrowed
  int nstage = 0, nb = 0;
  std::vector<double> A, c;
  long long ms = 0;  // member stride of the work arrays: 2·ncell
  DevBuf<double> ustart;
  std::vector<DevBuf<double>> ku;
  DevBuf<double> ub[2];
  DevBuf<double> pI;     // nb · n0 · n1
  DevBuf<double> phat;   // ROUTE_OWN2D: n1 · nb · kxs complex, [ky][member][kxs]
  DevBuf<double> zrows;  // nb zeros: the per-row part of the symbol in the fused y solve
  DevBuf<double> stats_part;  // ins_rk_ensemble_stats_f64: [member][chunk][3] workgroup partials, allocated on first use
};
// the checks an observer entry makes of one ensemble field and of the handle's box: INS_OK, an argument error, or the refusal that names the per-member calls
int ins_rk_ensemble_check_observer(const ins_rk_ensemble* e, const char* entry, long long ustride);
int ins_k_ownfft_xysolve2d_members(const ins_grid* G, const double* u, long long mstride, double* pI, int n0, int n1, int nb, const double* twx, const double* twy,
                                   const double* ax, const double* ay, hipStream_t s);
int ins_k_zsolve_members(double* data, int nz, long long nl, const double* ax, int kxn, const double* ay_rows, const double* az, const double* tw, double inv_n,
                         hipStream_t s, int kxs);
// rk->ub[0..1], allocated on first use: zeroed (init_from == nullptr, periodic loops) or a copy of init_from (tiled loops)   (ins_rk.hip)
int ins_rk_ensure_ub(ins_rk* rk, size_t bytes, hipStream_t s, const double* init_from);
// blocking reductions over an index box of a scalar field; op: 0 sum(a*b), 1 max|a|, 2 min(a)
int ins_k_reduce(const ins_grid* grid, int op, const double* a, const double* b, const int lo[3], const int hi[3], double* out,
                 hipStream_t s);

int ins_validate_real_plans(hipfftHandle fwd, hipfftHandle inv, int rank, const int* n, int batch);
int ins_fft_make_real_plans(hipfftHandle* fwd, hipfftHandle* inv, int rank, int* n, int batch);
void ins_fft_solver_released();
// side lengths the own passes take: a power of two in 16 .. 1024, or 3 * 2^m / 5 * 2^m (a radix-3 / radix-5 stage in front; INS_OWNFFT_POW2_ONLY
// leaves these to rocFFT)
static inline bool ins_pow2_len(int n) { return n >= 16 && n <= 1024 && !(n & (n - 1)); }
static inline bool ins_mixed_len(int n) {
  return (n == 96 || n == 192 || n == 384 || n == 160 || n == 320 || n == 640) && !ins_opt(OPT_INS_OWNFFT_POW2_ONLY);
}
// Where the x-forward pass (k_xfwd, ins_fft.hip) takes its rows from; the launchers carry it as `int from_u`, the kernels as template argument SRC.
enum XfwdSrc {
  XSRC_PI = 0,         // rows of the unpadded right-hand side pI
  XSRC_DIV = 1,        // Ω·div(u) formed on the fly, 3-D, periodic wrap in all directions
  XSRC_DIV_SLAB = 2,   // the same on a z-slab: the z neighbour comes from the ghost plane
  XSRC_DIV_2D = 3,     // Ω·div(u), 2-D, periodic wrap
  XSRC_DIV_WALLS = 4,  // Ω·div(u) on a grid with walls: the ghost volumes of u are valid
  XSRC_DIV_U32 = 5,    // as XSRC_DIV from a FLOAT velocity field, differences and metrics in double
  XSRC_FIELD = 6,      // one padded scalar array, ghosts stripped on the fly (observespectrum)
  XSRC_SPEC = 7,       // no x pass: the x-spectrum is already in phat (the stage kernel stored it, ins_flux64.hip XF); the solver's dispatcher only
};
bool ins_zsolve_supported(int nz);
bool ins_ownfft_supported(const int np[3]);
bool ins_ownfft_supported_slab(const int np[3]);
bool ins_ownfft_supported_mixed(const int np[3]);
void ins_ownfft_permute_symbol(int n, const double* ay, double* out);
// kxs: row stride of phat in complex elements (0 = dense, n0/2+1); a multiple of 8 keeps the y/z tiles 128-B aligned
// n2 planes starting at interior plane kz0
int ins_k_ownfft_xfwd(const ins_grid* G, const double* src, int from_u, double* phat, int n0, int n1, int n2, const double* tw, hipStream_t s,
                      int kxs = 0, int kz0 = 0);
int ins_k_ownfft_xinv(const double* phat, double* pI, int n0, int n1, int n2, const double* tw, hipStream_t s, int kxs = 0);
int ins_k_ownfft_y(double* phat, int kxn, int n1, int n2, const double* tw, bool inverse, hipStream_t s, int kxs = 0);
bool ins_ownfft_xy_supported(int n0, int n1);
int ins_k_ownfft_xy(const ins_grid* G, const double* src, int from_u, double* phat, double* pI, int n0, int n1, int n2, const double* twx, const double* twy,
                    bool inverse, hipStream_t s, int kxs);
int ins_k_ownfft_xysolve2d(const ins_grid* G, const double* src, int from_u, double* pI, int n0, int n1, const double* twx, const double* twy, const double* ax,
                           const double* ay, hipStream_t s);
bool ins_line3_supported(int n);
void ins_line3_permute_symbol(int n, const double* ay, double* out);
int ins_line3_pos_of_freq(int n, int k);
int ins_k_line3_z(double* phat, int kxn, int n1, int n2, const double* tw, hipStream_t s, int kxs);
int ins_k_line3_y(double* phat, int kxn, int n1, int n2, const double* tw, bool inverse, hipStream_t s, int kxs);
int ins_ownfft_yz_partitions(int kxn, int n1, int n2);
long long ins_ownfft_yz_scratch(int kxn, int n1, int n2, int P);
int ins_k_ownfft_yz_solve(double* phat, int kxn, int n1, int n2, int kxs, int P, const double* ax, const double* ay, double c, double scale, const double* tw_y,
                          double* scratch, hipStream_t s);
int ins_k_ownfft_y_packed(double* phat, double* packed, int kxn, int n1, int nzl, int nyl, int cw, const double* tw, bool inverse,
                          hipStream_t s);
int ins_zsolve_twiddles(int nz, DevBuf<double>* out);
int ins_k_fdm_z(double* data, int n0, int n1, int nz, const double* lx, const double* ly, const double* lz, const double* ox, const double* oy,
                double h, double tol, int singular, const double* meanf, double* partial, const double* tw, int* nblk, hipStream_t s, const double* dct_w = nullptr);
int ins_k_zsolve(double* data, int nz, long long nl, const double* ax, int kxn, const double* ay, const double* az, const double* tw,
                 double inv_n, bool zero_mean, hipStream_t s, int kxs = 0);

// communication used inside the library (ins_comm.hip): op 0 sum, 1 max, 2 min; scalar-field z ghost planes on a slab grid
int ins_comm_allreduce_internal(struct ins_comm* c, double* buf, long long count, int op, hipStream_t s);
int ins_comm_halo_scalar_internal(struct ins_comm* c, const ins_grid* G, double* p, hipStream_t s);

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
