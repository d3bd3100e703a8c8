// Model and primitive evaluation hooks (mhpc_eval_*): the model functions and the hand-written
// elementary functions as the solve's kernels call them, a point per lane.  Used by the tests
// only; no solve launches them.
#include <hip/hip_runtime.h>

#include "mhpc_device.h"
#include "mhpc_launch.h"
#include "mhpc_model_pair.h"

namespace MHPC_NS {

// ---- kernel-level parity hooks (batched CasADi replacements) -----------------------------
__global__ void k_eval_wb_dyn(int n, int mode, const real* x, const real* u, real* xd,
                              real* y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  wb_dynamics<real>(x + (size_t)i * 14, u + (size_t)i * 4, mode, xd + (size_t)i * 14, y + (size_t)i * 4);
}

// The line search's lane-pair dynamics (mhpc_model_pair.h): lane 2i + leg of point i, both
// lanes' xdot / y written ([n][2][14], [n][2][4]) so a test can check that each equals the
// single-lane model.  Lanes past 2n hold whole idle pairs (the DPP swaps stay inside pairs).
__global__ void k_eval_wb_dyn_pair(int n, int mode, const real* x, const real* u, real* xd,
                                   real* y) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = t >> 1;
  const bool back = t & 1;
  if (i >= n) return;
  const real* xi = x + (size_t)i * 14;
  const real u2[2] = {u[(size_t)i * 4 + (back ? 2 : 0)], u[(size_t)i * 4 + (back ? 3 : 1)]};
  real f[14], yy[4];
  wb_dynamics_pair(xi, u2, mode, back, f, yy);
  for (int r = 0; r < 14; ++r) xd[(size_t)t * 14 + r] = f[r];
  for (int r = 0; r < 4; ++r) y[(size_t)t * 4 + r] = yy[r];
}

// Touchdown constraint (WB_FL1/FL2_terminal_constr) as the kernels evaluate it: h both from
// the derivative routine (backward sweep) and from the value-only one (line search), hx, hxx;
// and the foot Jacobian (Jacob_F / Jacob_B) of the PD warm start.
__global__ void k_eval_wb_aux(int n, int foot, const real* x, real* h, real* hx, real* hxx,
                              real* J, real* Jd) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const real* xi = x + (size_t)i * 14;
  wb_touchdown(xi, foot, h + (size_t)i * 2, hx + (size_t)i * 14, hxx + (size_t)i * 196);
  h[(size_t)i * 2 + 1] = foot == kFront ? wb_touchdown_value<kFront>(xi) : wb_touchdown_value<kBack>(xi);
  wb_foot_jacobian(xi, foot, J + (size_t)i * 14, Jd + (size_t)i * 14);
}

__global__ void k_eval_wb_par(int n, int mode, const real* x, const real* u, real* Ac,
                              real* Bc, real* C, real* D) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 18) return;
  const int i = t / 18, dir = t % 18;
  // the partials kernel's method (implicit differentiation at the point's solution)
  real a[14], c[4];
  wb_partial_column(x + (size_t)i * 14, u + (size_t)i * 4, mode, dir, a, c);
  if (dir < 14) {
    for (int r = 0; r < 14; ++r) Ac[(size_t)i * 196 + r * 14 + dir] = a[r];
    for (int r = 0; r < 4; ++r) C[(size_t)i * 56 + r * 14 + dir] = c[r];
  } else {
    for (int r = 0; r < 14; ++r) Bc[(size_t)i * 56 + r * 4 + dir - 14] = a[r];
    for (int r = 0; r < 4; ++r) D[(size_t)i * 16 + r * 4 + dir - 14] = c[r];
  }
}

__global__ void k_eval_wb_impact(int n, int foot, const real* x, real* xp, real* Px) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 14) return;
  const int i = t / 14, dir = t % 14;
  Dual xx[14], yy[14], lam[2];
  for (int a = 0; a < 14; ++a) xx[a] = Dual(x[(size_t)i * 14 + a], a == dir ? real(1.0) : real(0.0));
  wb_impact<Dual>(xx, foot, yy, lam);
  for (int r = 0; r < 14; ++r) Px[(size_t)i * 196 + r * 14 + dir] = yy[r].d;
  if (dir == 0)
    for (int r = 0; r < 14; ++r) xp[(size_t)i * 14 + r] = yy[r].v;
}

__global__ void k_eval_srb(int n, const real* x, const real* u, const real* p,
                           const real* s, real* xd, real* Ac, real* Bc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  srb_dynamics(x + (size_t)i * 6, u + (size_t)i * 4, p + (size_t)i * 4, s + (size_t)i * 2, xd + (size_t)i * 6);
  srb_jacobians(x + (size_t)i * 6, u + (size_t)i * 4, p + (size_t)i * 4, s + (size_t)i * 2, Ac + (size_t)i * 36, Bc + (size_t)i * 24);
}

// One hand-written elementary function per point, called as the solve kernels call it
// (mhpc_eval_primitive, MHPC_PRIM_*).  Lane t of a 64-lane block evaluates point t of the
// launch, so the caller decides which arguments share a wave (the wave-uniform library
// fallback of sin_cos); of the sin_cos_n functions, group t of N consecutive angles.  out is
// [n][w]: w = 2 (sin, cos), 3 (B, Bz, Bzz) or 1.
template <int N>
static __device__ __forceinline__ void eval_sin_cos_n(int n, bool vk, const real* a, real* out) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  // the knot loops' VGPR copy of the constants (k_rollout); lanes past the last group run the
  // functions too, on zeros: the ballot inside is over the whole wave
  SinCosK scK = kSinCosK;
  if (vk) MHPC_PIN_VGPRS(scK);
  const bool live = (g + 1) * N <= n;
  real v[N], s[N], c[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = live ? a[(size_t)g * N + i] : real(0.0);
  if (vk) sin_cos_n<N>(v, s, c, scK);
  else sin_cos_n<N>(v, s, c);
  if (!live) return;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    out[((size_t)g * N + i) * 2] = s[i];
    out[((size_t)g * N + i) * 2 + 1] = c[i];
  }
}
__global__ void k_eval_prim(int fn, int n, const real* a, const real* b, real* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  switch (fn) {  // uniform
    case MHPC_PRIM_SINCOS_N5: eval_sin_cos_n<5>(n, false, a, out); return;
    case MHPC_PRIM_SINCOS_N3: eval_sin_cos_n<3>(n, false, a, out); return;
    case MHPC_PRIM_SINCOS_N5_VK: eval_sin_cos_n<5>(n, true, a, out); return;
    case MHPC_PRIM_SINCOS_N3_VK: eval_sin_cos_n<3>(n, true, a, out); return;
    default: break;
  }
  const bool live = i < n;
  const real ai = live ? a[i] : real(1.0);
  if (fn == MHPC_PRIM_SINCOS) {  // every lane of the wave reaches the ballot
    real s, c;
    sin_cos(ai, &s, &c);
    if (live) { out[(size_t)i * 2] = s; out[(size_t)i * 2 + 1] = c; }
    return;
  }
  if (!live) return;
  if (fn == MHPC_PRIM_PIVOT_RCP) {
    out[i] = pivot_rcp(ai);
  } else if (fn == MHPC_PRIM_LOG_POS) {
    out[i] = log_pos(ai);
  } else if (fn == MHPC_PRIM_REDUCED_BARRIER) {
    real B, Bz, Bzz;
    reduced_barrier(ai, b[i], &B, &Bz, &Bzz);
    out[(size_t)i * 3] = B; out[(size_t)i * 3 + 1] = Bz; out[(size_t)i * 3 + 2] = Bzz;
  } else if (fn == MHPC_PRIM_DIV_CONST) {  // b: 0 the SRB mass, otherwise its inertia
    out[i] = b[i] == real(0.0) ? div_const(ai, kSrbMass, kSrbMassRcp)
                               : div_const(ai, kSrbInertia, kSrbInertiaRcp);
  }
}

// ---- launchers (called by mhpc_runtime.cpp) ---------------------------------------------
hipError_t launch_eval_wb_dyn(int n, int mode, const real* x, const real* u, real* xd,
                              real* y, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_wb_dyn, dim3((n + 63) / 64), dim3(64), 0, s, n, mode, x, u, xd, y);
  return hipGetLastError();
}
hipError_t launch_eval_wb_dyn_pair(int n, int mode, const real* x, const real* u, real* xd,
                                   real* y, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_wb_dyn_pair, dim3((2 * n + 63) / 64), dim3(64), 0, s, n, mode, x, u, xd,
                     y);
  return hipGetLastError();
}
hipError_t launch_eval_wb_aux(int n, int foot, const real* x, real* h, real* hx, real* hxx,
                              real* J, real* Jd, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_wb_aux, dim3((n + 63) / 64), dim3(64), 0, s, n, foot, x, h, hx, hxx, J,
                     Jd);
  return hipGetLastError();
}
hipError_t launch_eval_wb_par(int n, int mode, const real* x, const real* u, real* Ac,
                              real* Bc, real* C, real* D, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_wb_par, dim3((n * 18 + 63) / 64), dim3(64), 0, s, n, mode, x, u, Ac,
                     Bc, C, D);
  return hipGetLastError();
}
hipError_t launch_eval_wb_impact(int n, int foot, const real* x, real* xp, real* Px,
                                 hipStream_t s) {
  hipLaunchKernelGGL(k_eval_wb_impact, dim3((n * 14 + 63) / 64), dim3(64), 0, s, n, foot, x, xp, Px);
  return hipGetLastError();
}
hipError_t launch_eval_srb(int n, const real* x, const real* u, const real* p,
                           const real* c, real* xd, real* Ac, real* Bc, hipStream_t s) {
  hipLaunchKernelGGL(k_eval_srb, dim3((n + 63) / 64), dim3(64), 0, s, n, x, u, p, c, xd, Ac, Bc);
  return hipGetLastError();
}
int eval_prim_group(int fn) {
  return fn == MHPC_PRIM_SINCOS_N5 || fn == MHPC_PRIM_SINCOS_N5_VK   ? 5
         : fn == MHPC_PRIM_SINCOS_N3 || fn == MHPC_PRIM_SINCOS_N3_VK ? 3
                                                                     : 1;
}
hipError_t launch_eval_prim(int fn, int n, const real* a, const real* b, real* out,
                            hipStream_t s) {
  const int lanes = n / eval_prim_group(fn);  // n is a multiple of the group (the hook checks)
  hipLaunchKernelGGL(k_eval_prim, dim3((lanes + 63) / 64), dim3(64), 0, s, fn, n, a, b, out);
  return hipGetLastError();
}

}  // namespace MHPC_NS
