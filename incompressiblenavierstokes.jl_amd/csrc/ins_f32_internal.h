// Internal launchers of the `_f32` family used across translation units (stream-ordered, non-blocking), grouped by the file that defines them.
#pragma once

#include "ins_internal.h"

// Launch sequence of a Float32 solver: chosen once, when the solver is created (ins_f32_choose / ins_poisson_wrap_f32, ins_f32.hip), stored in the handle and
// dispatched on by ins_project_f32, ins_poisson_solve_f32, ins_max_abs_divergence_f32 and the step's route (rk32_route).  A new route is a new value here.
enum F32Route {
  F32_HIPFFT = 0,      // Ω·div(u) -> hipFFT R2C -> symbol -> C2R in float, then pad -> gradient-subtract -> periodic ghosts
  F32_FP64_SPECTRA,    // 3-D boxes whose fp64 solver runs on own passes: those passes, fed from the float field
  F32_FLOAT2_SPECTRA,  // of those, the z sides of the three-pass z kernel (192, 256, 384, 512): the same passes on float2 spectra
  F32_WRAP,            // a caller-owned fp64 solver of any kind (ins_poisson_wrap_f32): walls, stretched spacings
};
// ins_f32.hip: the route of an all-periodic uniform box under the option values at the time of the call (no device); never F32_WRAP
F32Route ins_f32_choose(int D, int n0, int n1, int n2);
// the wrapped fp64 solver of a Float32 solver handle (nullptr: not on F32_WRAP) with its padded fp64 scratch, and the handle's grid
ins_poisson* ins_k32_wrapped(const ins_poisson32* ps, double** p64);
const ins_grid* ins_k32_solver_grid(const ins_poisson32* ps);
// out = base + Σ_q coef[q]·k[q] over n floats, terms in index order (k32_combine)
int ins_k32_combine(long long n, const float* base, float* out, int nterms, const float* coef, const float* const* k, hipStream_t s);

// ins_f32g.hip: the operators on any grid (walls, stretched spacings, 2-D or 3-D), boundary data constant
int ins_k32g_apply_bc_u(const ins_grid* G, float* u, hipStream_t s, int dudt = 0);
int ins_k32g_apply_bc_p(const ins_grid* G, float* p, hipStream_t s);
int ins_k32g_apply_bc_p_fields(const ins_grid* G, float* p, int nf, hipStream_t s);  // nf scalar fields back to back, one launch per direction
int ins_k32g_momentum(const ins_grid* G, float visc, const float* u, float* F, hipStream_t s);
int ins_k32g_divergence(const ins_grid* G, const float* u, float* div, hipStream_t s);  // div[Ip] = divergence(u); volumes outside Ip are left as they are
// psolver(p) with a Float32 p around the fp64 solver (widen, solve, round; p64: padded fp64 scratch), and project! on it
int ins_k32g_solve(const ins_grid* G, ins_poisson* ps64, double* p64, float* p, hipStream_t s);
int ins_k32g_project(const ins_grid* G, ins_poisson* ps64, double* p64, float* u, float* p, hipStream_t s);

// ins_temp32.hip: diff = diffusion(u) on the degrees of freedom, zero elsewhere; one stage of the temperature equation (diff nullable; ks: the previous ktemp_j)
int ins_k32t_diffusion(const ins_grid* G, float visc, const float* u, float* diff, hipStream_t s);
int ins_k32t_stage(const ins_grid* G, float a4, float coef, const float* u, const float* temp, const float* diff, const float* tempstart, int n,
                   const float* coefs, const float* const* ks, float c_self, float* ktemp_out, float* temp_out, hipStream_t s);

// ins_smagforce32.hip: the Smagorinsky closure force in one kernel (grids: ins_smagforce_supported); u with its boundary data applied
int ins_k_smagforce_f32(const ins_grid* G, float theta, const float* u, float* sout, hipStream_t s);

// ins_tensorclosure32.hip: pass 2 of the tensor-basis pullbacks, ubar (+)= ∇ᵀ of the ∇ubar scratch gb read as floats
int ins_k32_gradu_adjoint(const ins_grid* G, const float* gb, float* ubar, bool accumulate, hipStream_t s);

// ins_flux64.hip, ins_flux128.hip: the stage kernels instantiated for float; RkEpi's pointers are float arrays then
int ins_k_flux64_f32(const ins_grid* G, double visc, const float* u, float* F, const RkEpi* epi, const float* pI, int corr_mode, hipStream_t s, int part = 0);
int ins_k_flux128_f32(const ins_grid* G, double visc, const float* u, float* F, const RkEpi* epi, const float* pI, int corr_mode, hipStream_t s, int part);

// ins_fft.hip, ins_zsolve.hip: the own passes on float2 spectra (half the bytes); tw = float2 twiddles (ins_zsolve_twiddles_f32), symbols stay double
int ins_k_ownfft_xfwd_f32(const ins_grid* G, const float* src, int from_u, float* phat, int n0, int n1, int n2, const float* tw, hipStream_t s, int kxs);
int ins_k_ownfft_xinv_f32(const float* phat, float* pI, int n0, int n1, int n2, const float* tw, hipStream_t s, int kxs);
int ins_k_ownfft_y_f32(float* phat, int kxn, int n1, int n2, const float* tw, bool inverse, hipStream_t s, int kxs);
int ins_k_line3_y_f32(float* phat, int kxn, int n1, int n2, const float* tw, bool inverse, hipStream_t s, int kxs);
bool ins_zsolve_f32_supported(int nz);
int ins_zsolve_twiddles_f32(int nz, DevBuf<float>* out);
int ins_k_zsolve_f32(float* data, int nz, long long nl, const double* ax, int kxn, const double* ay, const double* az, const float* tw, double inv_n,
                     bool zero_mean, hipStream_t s, int kxs);

// ins_poisson.hip: a periodic 3-D box's pressure equation on the fp64 solver's own passes, Ω·div(u) from the float field u32, solution in its pI (double) ...
int ins_k_spectral_solve_from_u32(ins_poisson* ps, const float* u32, hipStream_t s);
const double* ins_k_spectral_pI(const ins_poisson* ps);
// ... and the same five passes on float2 spectra: ps supplies the symbol vectors and the grid, the float work arrays and twiddles are the caller's.
// u32 == nullptr: the right-hand side is in pI32.  Solution in pI32 (unpadded)
bool ins_k_spectral_own3d_f32(const ins_poisson* ps);
int ins_k_spectral_solve_f32(ins_poisson* ps, const float* u32, float* pI32, float* phat32, int kxs32, const float* twx, const float* twy,
                             const float* twz, hipStream_t s);
