// The temperature equation of the `_f32` family (T = Float32; examples/RayleighBenard2D.jl:71 and examples/RayleighBenard3D.jl:16 run it in single precision):
// the temperature kernels of csrc/ins_fields.hip and csrc/ins_temp_kernels.h (which cite the reference lines) in float, on ANY grid the fp64 ones take — 2-D / 3-D, periodic,
// Dirichlet, symmetric and pressure temperature sides, uniform and stretched spacings.
//
//   fields      : Float32 arrays in the reference layout; the grid handle is the fp64 one, metric tables are read as doubles and rounded to float where they
//                 enter the arithmetic (as csrc/ins_f32g.hip); all arithmetic in float;
//   operators   : apply_bc_temp!, convection_diffusion_temp! (c += ...), dissipation! (diss += ...; needs a float diffusion! alone, k32t_diffusion),
//                 gravity! (F[:, gdir] += ...): the write sets, += rules and BC codes of the `_f64` entries; boundary data constant (no plane buffers).
//                 k_bc_temp, k_gravity and k_dissipation_interp are the float instantiations of csrc/ins_temp_kernels.h;
//   kept copies : k32t_convdiff_temp and k32t_stage (of k_convdiff_temp and k_temp_stage without its in-kernel pressure correction and `w` input,
//                 csrc/ins_fields.hip): the same arithmetic, but no spelling tried reproduces the instruction schedule of both precisions
//                 (profiles/forward_generic_isa.md lists them); k32t_diffusion (of k_convdiff<D, 2, true>): other FMA contraction, see k32g_momentum in
//                 csrc/ins_f32g.hip.  A fix to one of these goes into its fp64 twin as well;
//   stage kernel: one pass over Ip forms ktemp_i = convection_diffusion_temp(u, temp) + dissipation(u) and temp_out = tempstart + Σ_j Δt A[i,j] ktemp_j
//                 (k32t_stage); the stage loop that calls it is ins_rk_step_ext_f32 (csrc/ins_f32.hip, beside the isothermal loop whose handle it extends).
// Slab (HALO) sides are not taken: the multi-GPU path is fp64.
#include "ins_f32_internal.h"
#include "ins_temp_kernels.h"

namespace {

// avg(ϕ, Δ, I, α) with float weights                                            operators.jl:59-62
__device__ __forceinline__ float avg32(float d0, float d1, float p0, float p1) { return (d1 * p0 + d0 * p1) / (d0 + d1); }

// One direction of convection_diffusion_temp! at volume c (index ib along b): (-(uT2 - uT1) + α4 (dT2 - dT1)) / Δ      operators.jl:712-737
__device__ __forceinline__ float convdiff_temp_dir(const GridDev& g, int b, int ib, float a4, float u1, float u2, float tm, float tc, float tp) {
  const float dm = (float)g.dx[b][ib - 1], d0 = (float)g.dx[b][ib], dp = (float)g.dx[b][ib + 1];
  const float dT1 = (tc - tm) * (float)g.rdxu[b][ib - 1];
  const float dT2 = (tp - tc) * (float)g.rdxu[b][ib];
  const float uT1 = u1 * avg32(dm, d0, tm, tc);
  const float uT2 = u2 * avg32(d0, dp, tc, tp);
  return (-(uT2 - uT1) + a4 * (dT2 - dT1)) * (float)g.rdx[b][ib];
}

// convection_diffusion_temp!  (c += ...)                                        operators.jl:712-737
template <int D>
__global__ __launch_bounds__(256) void k32t_convdiff_temp(GridDev g, BoxMap L, float a4, const float* __restrict__ u, const float* __restrict__ temp,
                                                          float* __restrict__ out) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
  const float tc = temp[c];
  float acc = 0.f;
#pragma unroll
  for (int b = 0; b < D; ++b) {
    const long long sb = g.sx[b];
    const float* ub = u + b * g.sc;
    acc += convdiff_temp_dir(g, b, I[b], a4, ub[c - sb], ub[c], temp[c - sb], tc, temp[c + sb]);
  }
  out[c] += acc;
}

// fill!(diff, 0); diffusion!(diff, u, setup) in one write-only pass over the padded array: the diffusion term on the degrees of freedom of each component,
// zero elsewhere (operators.jl:793-794, 565-607).  The diffusive part of k32g_momentum, term by term.
template <int D>
__global__ __launch_bounds__(256) void k32t_diffusion(GridDev g, float visc, const float* __restrict__ u, float* __restrict__ F) {
  INS_VOL_INDEX(g.sx, 0, 0, 0, i >= g.N[0] || j >= g.N[1]);
#pragma unroll
  for (int al = 0; al < D; ++al) {
    float* Fa = F + al * g.sc;
    if (!dof<D>(g, al, i, j, k)) {
      Fa[c] = 0.f;
      continue;
    }
    const float* ua = u + al * g.sc;
    const float uc = ua[c];
    float f = 0.f;
#pragma unroll
    for (int be = 0; be < D; ++be) {
      const long long sb = g.sx[be];
      const int ib = I[be];
      const float um = ua[c - sb], up = ua[c + sb];
      const float r = (float)(al == be ? g.rdxu[be] : g.rdx[be])[ib];
      const float ma = (float)(al == be ? g.mdx[be][ib] : g.mdxu[be][ib - 1]);
      const float mb = (float)(al == be ? g.mdx[be][ib + 1] : g.mdxu[be][ib]);
      f += visc * ((up - uc) * mb - (uc - um) * ma) * r;
    }
    Fa[c] = f;
  }
}

// One stage of the temperature equation in one pass over Ip (ins_rk_step_ext_f32; step_explicit_runge_kutta.jl:23-27, 39-44):
//   ktemp_i  = convection_diffusion_temp(u, temp) + coef · Σ_β (u_β diff_β at the two faces) / 2        (diff = diffusion(u): zero off the DOFs; nullable)
//   temp_out = tempstart + Σ_j c_j ktemp_j + c_self ktemp_i
// instead of fill!, convection_diffusion_temp!, the interpolation kernel of dissipation! and the combination.  Per volume and direction it loads two faces of
// u and of diff and two neighbours of temp (unit-stride rows; the y / z neighbours come from the rows and planes the XCD band has just read); temp_out is
// another array than temp (neighbours of temp are read here).  ktemp_i is stored only when a later stage reads it.
struct TempStage32 {
  int n;
  float coef[INS_MAX_STAGES];
  const float* k[INS_MAX_STAGES];
  float c_self;
  const float* tempstart;
  float* ktemp_out;  // nullable
  float* temp_out;
};
template <int D>
__global__ __launch_bounds__(256) void k32t_stage(GridDev g, BoxMap L, float a4, float coef, const float* __restrict__ u, const float* __restrict__ temp,
                                                  const float* __restrict__ diff, TempStage32 ts) {
  INS_BANDED_INDEX(g.ip_lo[0], g.ip_lo[1], g.ip_lo[2], g.ip_hi[0], g.ip_hi[1]);
  const float tc = temp[c];
  float acc = 0.f, d = 0.f;
#pragma unroll
  for (int b = 0; b < D; ++b) {
    const long long sb = g.sx[b];
    const float* ub = u + b * g.sc;
    const float u1 = ub[c - sb], u2 = ub[c];
    acc += convdiff_temp_dir(g, b, I[b], a4, u1, u2, temp[c - sb], tc, temp[c + sb]);
    if (diff) {
      const float* db = diff + b * g.sc;
      d += coef * (u1 * db[c - sb] + u2 * db[c]) / 2;
    }
  }
  acc += d;
  float t = ts.tempstart[c];
  for (int q = 0; q < ts.n; ++q) t += ts.coef[q] * ts.k[q][c];
  t += ts.c_self * acc;
  if (ts.ktemp_out) ts.ktemp_out[c] = acc;
  ts.temp_out[c] = t;
}

inline Launch3 ip_launch(const GridDev& g) { return banded_launch(g.D, g.ip_lo, g.ip_hi); }

}  // namespace

// ------------------------------------------------------------------------------------------------ internal launchers (csrc/ins_f32.hip)
// diff = diffusion(u) on the degrees of freedom, zero elsewhere
int ins_k32t_diffusion(const ins_grid* G, float visc, const float* u, float* diff, hipStream_t s) {
  const GridDev& g = G->g;
  INS_LAUNCH_D((k32t_diffusion<D>), box_launch(g.D, g.N), s, g, visc, u, diff);
  return INS_OK;
}

// diff nullable (no dissipation term); ks / coefs: the previous ktemp_j (terms with a zero coefficient are dropped)
int ins_k32t_stage(const ins_grid* G, float a4, float coef, const float* u, const float* temp, const float* diff, const float* tempstart, int n,
                   const float* coefs, const float* const* ks, float c_self, float* ktemp_out, float* temp_out, hipStream_t s) {
  const GridDev& g = G->g;
  TempStage32 ts;
  ts.n = 0;
  for (int q = 0; q < n && ts.n < INS_MAX_STAGES; ++q) {
    if (coefs[q] == 0.f) continue;
    ts.coef[ts.n] = coefs[q];
    ts.k[ts.n] = ks[q];
    ++ts.n;
  }
  ts.c_self = c_self;
  ts.tempstart = tempstart;
  ts.ktemp_out = ktemp_out;
  ts.temp_out = temp_out;
  Launch3 l = ip_launch(g);
  INS_LAUNCH_D((k32t_stage<D>), l, s, g, l.map, a4, coef, u, temp, diff, ts);
  return INS_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int ins_apply_bc_temp_f32(const ins_grid_t* G, const int32_t* bc, const float* val, float* temp, void* stream) {
  INS_REQUIRE(G && bc && val && temp, "null argument");
  const GridDev& g = G->g;
  int rc = no_halo(G, "ins_apply_bc_temp_f32");
  if (rc) return rc;
  for (int be = 0; be < g.D; ++be) {  // direction after direction, as apply_bc_temp!: edges and corners come out as in the reference
    TempBC<float> t;
    for (int side = 0; side < 2; ++side) {
      t.bc[side] = bc[2 * be + side];
      t.val[side] = val[2 * be + side];
      t.plane[side] = nullptr;  // constant boundary data
      INS_REQUIRE(t.bc[side] == INS_BC_PERIODIC || t.bc[side] == INS_BC_DIRICHLET || t.bc[side] == INS_BC_SYMMETRIC || t.bc[side] == INS_BC_PRESSURE,
                  "temperature boundary condition");
    }
    INS_REQUIRE((t.bc[0] == INS_BC_PERIODIC) == (t.bc[1] == INS_BC_PERIODIC), "periodic on both sides");
    INS_LAUNCH_D((k_bc_temp<D, float>), line_launch(g, be, 1), as_stream(stream), g, temp, be, t);
  }
  return INS_OK;
}

extern "C" int ins_convection_diffusion_temp_f32(const ins_grid_t* G, float a4, const float* u, const float* temp, float* c, void* stream) {
  INS_REQUIRE(G && u && temp && c, "null argument");
  const GridDev& g = G->g;
  int rc = no_halo(G, "ins_convection_diffusion_temp_f32");
  if (rc) return rc;
  Launch3 l = ip_launch(g);
  INS_LAUNCH_D((k32t_convdiff_temp<D>), l, as_stream(stream), g, l.map, a4, u, temp, c);
  return INS_OK;
}

extern "C" int ins_dissipation_f32(const ins_grid_t* G, float visc, float coef, const float* u, float* diff, float* diss, void* stream) {
  INS_REQUIRE(G && u && diff && diss, "null argument");
  INS_REQUIRE(u != diff, "diffusion! cannot run in place");
  const GridDev& g = G->g;
  int rc = no_halo(G, "ins_dissipation_f32");
  if (rc) return rc;
  if ((rc = ins_k32t_diffusion(G, visc, u, diff, as_stream(stream)))) return rc;  // fill!(diff, 0); diffusion!(diff, u, setup)     operators.jl:797-798
  Launch3 l = ip_launch(g);
  INS_LAUNCH_D((k_dissipation_interp<D, float>), l, as_stream(stream), g, l.map, coef, u, (const float*)diff, diss);
  return INS_OK;
}

extern "C" int ins_gravity_f32(const ins_grid_t* G, int gdir, float a2, const float* temp, float* F, void* stream) {
  INS_REQUIRE(G && temp && F, "null argument");
  const GridDev& g = G->g;
  INS_REQUIRE(gdir >= 0 && gdir < g.D, "gravity direction");
  int rc = no_halo(G, "ins_gravity_f32");
  if (rc) return rc;
  Launch3 l = banded_launch(g.D, g.iu_lo[gdir], g.iu_hi[gdir]);
  INS_LAUNCH_D((k_gravity<D, float>), l, as_stream(stream), g, l.map, gdir, a2, temp, F);
  return INS_OK;
}
