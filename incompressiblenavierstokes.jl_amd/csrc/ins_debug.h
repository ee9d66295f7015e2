// Experiment / test hooks the library exports beside include/ins_hip.h: not part of the public ABI.  The tests and the labs under tools/ call them through
// ctypes; the translation units that define them include this header, so every definition is checked against the one declaration here.
#pragma once

#include <stdint.h>

#include "ins_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ins_fast3d.hip, ins_fast3d_flux.hip, ins_flux64.hip.  Tuning knobs for experiments in one process on one allocation, not part of the public ABI
 * (flux64: -1 keeps a value) */
void ins_tune_fast3d(int rows, int zchunk);
void ins_tune_flux3d(int rows, int zchunk, int xw);
void ins_tune_flux64(int disable, int rows, int rows_corr, int zchunk, int xw, int skel, int burst_unused, int lds);

/* ins_poisson.hip.  Test hook, not part of the public ABI: which directions of the direct solver run in trigonometric modes (1 Fourier z, 2 Fourier x,
 * 4 Fourier x and y, 8 cosine z); -1: not a direct solver */
int ins_dbg_fdm_modes(const ins_poisson_t* ps);
/* experiment / test hook, not part of the public ABI: which directions of a direct solver run as folded half-size GEMMs (bit a = direction a) */
int ins_dbg_fdm_fold_mask(const ins_poisson_t* ps);
/* test hooks, not part of the public ABI: a live spectral solver's route and ky order (SpectralRoute / KyOrder values; -1: not a spectral solver); the choice
 * for a box under the current option values, without touching the device; the symbol permutation of a ky order and the inverse map of the k_line3 one */
int ins_dbg_spectral_route(const ins_poisson_t* ps, int32_t* ky_order);
int ins_dbg_spectral_choose(int D, int n0, int n1, int n2, int32_t* ky_order, int32_t* partitions);
void ins_dbg_permute_ky(int ky_order, int n, const double* ay, double* out);
int ins_dbg_line3_pos_of_freq(int n, int k);

/* ins_f32.hip.  Test hooks, not part of the public ABI: the Float32 solver route (F32Route of csrc/ins_f32_internal.h) of an all-periodic uniform box of
 * n0 x n1 (x n2) volumes under the current option values, without touching the device; a live Float32 integrator's solver route, and in *flags its step
 * route as a bit set (1 general, 2 wide, 4 in-register correction, 8 float2 spectra, 16 stage-velocity basis, 32 chainable) */
int ins_dbg_f32_choose(int D, int n0, int n1, int n2);
int ins_dbg_rk32_route(const ins_rk32_t* rk, int32_t* flags);

/* ins_zsolve.hip.  Experiment hook, not part of the public ABI: time `reps` launches of the fused z pass on `data` = nbox independent [nz][nl] blocks
 * (nl = nky * kxs lines, kxn live columns), average ms per sweep over all boxes */
int ins_dbg_zsolve(double* data, int nz, long long nl, int kxn, int kxs, int nbox, int reps, float* ms);

/* ins_rk.hip.  Test hook, not part of the public ABI (needs no device): the carry plan of the caller's tableau.  *j < 0: no plan.  With a plan: a[3], and the
 * consuming stage's terms: *self_in, *coef_self and *coef_force (0 without a force) */
int ins_dbg_rk_carry_plan(int32_t ns, const double* A, double dt, int32_t with_force, int32_t* j, int32_t* i, double* a, double* self_in, double* coef_self,
                          double* coef_force);
/* test hook, not part of the public ABI (needs no device): the stage-term builders on the caller's tableau.  kind 0 / 1: the k-basis / the stage-velocity
 * basis (order 0: force sum diagonal first, 1: index order); kind 2 / 3: the plain sum in double / float.  stage[q], coef[q]: room for INS_MAX_STAGES + 1 */
int ins_dbg_rk_stage_terms(int32_t ns, const double* A, int32_t i, double dt, int32_t kind, int32_t input_in_regs, int32_t with_force, int32_t order,
                           int32_t* n, int32_t* stage, double* coef, double* c0m1, double* self_in, double* coef_self, int32_t* write_k, double* coef_force);
/* test / lab hook, not part of the public ABI: how many steps this integrator's cache has run as graph replays */
long long ins_dbg_rk_graph_replays(const ins_rk_t* rk);

/* ins_rk_ensemble.hip.  Test hook, not part of the public ABI (needs no device): the argument checks ins_rk_ensemble_create and ins_rk_ensemble_steps_f64 make
 * once they know the grid's ncell — the member count, the step count and the member stride */
int ins_dbg_rk_ensemble_args(int64_t ncell, int32_t nbatch, int64_t ustride, int32_t nsteps);

/* ins_rk_ext.hip.  Test hooks, not part of the public ABI: how many steps of the extended stage loop took the tiled / the fused path */
long long ins_dbg_ext_tiled_steps(void);
long long ins_dbg_ext_fused_steps(void);

/* ins_devmem.hip.  Test hook, not part of the public ABI: device and pinned-host buffers the library holds at this moment, and their bytes (either
 * pointer may be NULL).  A handle that has been destroyed holds none. */
void ins_dbg_dev_live(int64_t* buffers, int64_t* bytes);

#ifdef __cplusplus
}
#endif
